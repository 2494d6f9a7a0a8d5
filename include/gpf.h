/*
 * gpf.h -- C ABI of libgpf_hip.so: the MI355X (gfx950) particle-filter hot path behind the
 * pf_initialize / pf_update! / pf_resample! / pf_rejuvenate! API of GenParticleFilters.jl.
 *
 * The reference has no FFI: its boundary is Julia multiple dispatch on
 * ParticleFilterView (reference src/view.jl:32-33).  A drop-in therefore is a new state type
 * whose methods ccall the entry points below (julia/GenParticleFiltersAMD.jl).
 * Every entry point names the reference method it replaces (paths relative to the reference
 * repository root, v0.2.3).
 *
 * Conventions
 *   - plain C types only; no C++/torch types cross this boundary.
 *   - every function returns a gpf_status; nothing throws across the ABI.  The Julia glue maps
 *     a non-zero status to error(gpf_last_error(h)) (ErrorException, like the reference's error()).
 *   - the handle owns all device buffers; host arrays passed in or out belong to the caller.
 *   - one handle = one host thread at a time.  Work is enqueued on one HIP stream; calls that
 *     return a scalar or fill a host array synchronise that stream, all others are asynchronous.
 *   - particle state is Float64; ancestor indices are reported 1-based Int64 into the
 *     PRE-resample particle array, exactly like state.parents (reference test/resample.jl:11).
 *   - there is no CPU fallback: gpf_create fails if no gfx950 device is usable.
 */
#ifndef GPF_H
#define GPF_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#define GPF_ABI_VERSION 1

typedef struct gpf_filter* gpf_handle;

/* the library is built with -fvisibility=hidden: the functions this header declares are what it exports */
#pragma GCC visibility push(default)

typedef enum {
    GPF_OK = 0,
    GPF_ERR_INVALID_ARGUMENT = 1,
    GPF_ERR_INVALID_WEIGHTS = 2,   /* error("Invalid weights.")            src/resample.jl:55,92,151 */
    GPF_ERR_UNKNOWN_METHOD = 3,    /* error("... method ... not recognized") src/resample.jl:28, src/rejuvenate.jl:25 */
    GPF_ERR_HIP = 4,               /* a HIP runtime call failed; see gpf_last_error */
    GPF_ERR_NO_DEVICE = 5,
    GPF_ERR_STATE = 6              /* operation not valid in the current state (e.g. update before initialize) */
} gpf_status;

/* native models (the reference runs arbitrary Gen programs; the hot path runs these compiled ones) */
typedef enum {
    GPF_MODEL_LGSSM2 = 1,          /* 2-D linear-Gaussian SSM              (BASELINE configs 2,3) */
    GPF_MODEL_BEARINGS4 = 2,       /* bearings-only tracking, 4-D          (BASELINE config 4)   */
    GPF_MODEL_SV1 = 3,             /* stochastic volatility, 1-D           (BASELINE config 5)   */
    GPF_MODEL_OBJECT_MOTION = 4,   /* reference README.md:43-55            (BASELINE config 1)   */
    GPF_MODEL_LINE = 5             /* line_model, the fixture of the reference's tests (test/runtests.jl:3-16) */
} gpf_model;

/* method::Symbol of pf_resample! (src/resample.jl:19-30) */
typedef enum { GPF_RESAMPLE_MULTINOMIAL = 0, GPF_RESAMPLE_RESIDUAL = 1, GPF_RESAMPLE_STRATIFIED = 2,
               GPF_RESAMPLE_OPTIMAL = 3 /* gpf_resize only: pf_optimal_resize!, src/resize.jl:149-219 */,
               /* OPT-IN extension, not a reference method: pf_multinomial_resample! (src/resample.jl:48-65) with the N uniforms drawn
                * ALREADY SORTED (uniform spacings in exact integers).  Offspring counts ~ Multinomial(N, w) as for :multinomial;
                * state.parents comes out non-decreasing instead of as an i.i.d. sequence (src/resample.jl:59), so slot k of the new
                * population is NOT exchangeable with slot k' any more -- harmless for a filter that treats its particles as a set, visible
                * to code that cuts the population into views by position.  The ancestor search becomes a streaming merge and the row
                * gather reads ascending rows.  gpf_resample (and views) only.  Invalid weights (all -Inf, the uniform fallback): the targets
                * are placed on the grid of N 2^K, not of S = N, so that every particle is drawn with probability 1 / N. */
               GPF_RESAMPLE_MULTINOMIAL_SORTED = 4 } gpf_resample_method;
/* method::Symbol of pf_rejuvenate! (src/rejuvenate.jl:18-27) */
typedef enum { GPF_REJUVENATE_MOVE = 0, GPF_REJUVENATE_REWEIGHT = 1 } gpf_rejuvenate_method;
/* check keyword of the resamplers: true | :warn | false (src/resample.jl:43-46) */
typedef enum { GPF_CHECK_FALSE = 0, GPF_CHECK_WARN = 1, GPF_CHECK_TRUE = 2 } gpf_check;

typedef struct {
    int32_t  abi_version;    /* GPF_ABI_VERSION */
    int32_t  model;          /* gpf_model */
    int32_t  n_params;       /* <= 24 */
    int32_t  keep_prev;      /* 1: rows also carry x_{t-1} (needed by gpf_rejuvenate) */
    const double* params;    /* model parameters, layout in csrc/gpf_models.hpp */
    int64_t  n_particles;    /* particles held by this handle (this shard) */
    int64_t  n_global;       /* particles of the whole filter; == n_particles when unsharded */
    int64_t  gid0;           /* global index of local particle 0 (RNG counters use global ids) */
    uint64_t seed;           /* Philox key */
    int32_t  device;         /* HIP device ordinal */
    int32_t  reserved;
    void*    stream;         /* hipStream_t to enqueue on, or NULL for a library-owned stream */
} gpf_config;

/* ---- lifetime ------------------------------------------------------------------------------ */
int  gpf_abi_version(void);
gpf_status gpf_create(const gpf_config* cfg, gpf_handle* out);
gpf_status gpf_destroy(gpf_handle h);
const char* gpf_last_error(gpf_handle h);         /* valid until the next call on h; h may be NULL */
gpf_status gpf_synchronize(gpf_handle h);

/* ---- the four operations ------------------------------------------------------------------- */
/* pf_initialize(model, model_args, observations, n_particles)      src/initialize.jl:31-44
 * x_1 ~ prior, log_weights[i] = log p(obs | x_1), log_ml_est = 0, parents = 1:N. */
gpf_status gpf_initialize(gpf_handle h, const double* obs, int32_t n_obs);

/* pf_update!(state, new_args, argdiffs, observations)              src/update.jl:12-25
 * x_t ~ p(. | x_{t-1}), log_weights[i] += log p(obs | x_t); buffers swap (update_refs!, src/utils.jl:10-15). */
gpf_status gpf_update(gpf_handle h, const double* obs, int32_t n_obs);

/* One iteration of the reference's README loop (README.md:66-77) in one call:
 *     if effective_sample_size(state) < ess_frac * N   (src/utils.jl:163-164)
 *         pf_resample!(state, resample_method; check, sort_particles)          (src/resample.jl:19-30)
 *         pf_rejuvenate!(state, kern, (), n_iters; method = rejuvenate_method)  (src/rejuvenate.jl:18-27; rejuvenate_method < 0: none)
 *     end
 *     pf_update!(state, new_args, argdiffs, observations)                       (src/update.jl:12-25)
 * Same results as the four calls in that order, bit for bit.  The ESS verdict is also formed on the device and the propagate is
 * enqueued speculatively behind it, so the steps that do not resample never wait for the host's decision.
 * resampled / invalid / ess_out may be NULL. */
gpf_status gpf_step_ess(gpf_handle h, const double* obs, int32_t n_obs, double ess_frac, int32_t resample_method, int32_t sort_particles,
                        int32_t check, int32_t rejuvenate_method, int32_t n_iters, int32_t* resampled, int32_t* invalid, double* ess_out);

/* pf_initialize(model, args, obs, proposal, proposal_args, n)        src/initialize.jl:46-62
 * pf_update!(state, new_args, argdiffs, obs, proposal, proposal_args) src/update.jl:79-96 (+ src/translate.jl:86-105)
 * with a NATIVE proposal: new latents x ~ q(. | x_{t-1}, y_t); log_weights[i] += [log p(x | x_{t-1}) + log p(y | x)] - log q(x).
 * GPF_PROPOSAL_LOCALLY_OPTIMAL: the exact conditional of the linear-Gaussian model (GPF_MODEL_LGSSM2 only).
 * GPF_PROPOSAL_LINE_FIXED: the proposals of the reference's own tests for GPF_MODEL_LINE, slope ~ uniform_discrete(0, 0) at
 * the first step and outlier ~ bernoulli(0.0) at every step (test/initialize.jl:16-19, test/update.jl:42-43). */
typedef enum { GPF_PROPOSAL_LOCALLY_OPTIMAL = 1, GPF_PROPOSAL_LINE_FIXED = 2 } gpf_proposal;
gpf_status gpf_initialize_proposal(gpf_handle h, const double* obs, int32_t n_obs, int32_t proposal);
gpf_status gpf_update_proposal(gpf_handle h, const double* obs, int32_t n_obs, int32_t proposal);

/* Stratified initialisation / update over a discrete latent          src/initialize.jl:92-109, src/update.jl:193-210,
 * stratified_map! src/utils.jl:29-55.  values[k] = the value the model's discrete latent is constrained to in stratum k
 * (GPF_MODEL_OBJECT_MOTION: `moving`, 0 or 1); K = n_strata <= 8, block size B = n div K; particle i < K B belongs to
 * stratum i div B (interleaved = 0, :contiguous) or i mod K (interleaved = 1); the remaining particles draw their stratum
 * uniformly.  log_weights[i] (+)= log p(latent = value | parents) + log p(obs | x) + log K. */
gpf_status gpf_initialize_strata(gpf_handle h, const double* obs, int32_t n_obs, const double* values, int32_t n_strata, int32_t interleaved);
gpf_status gpf_update_strata(gpf_handle h, const double* obs, int32_t n_obs, const double* values, int32_t n_strata, int32_t interleaved);
/* pf_initialize(model, args, obs, strata, proposal, proposal_args, n; layout)   src/initialize.jl:111-129: the stratified latent is
 * constrained per stratum, the model's other choice comes from a native proposal, log_weights[i] = model_weight - prop_weight +
 * log(n_strata).  GPF_MODEL_LINE with GPF_PROPOSAL_LINE_FIXED: strata over `slope`, outlier ~ bernoulli(0.0) -- the form the reference
 * tests (test/initialize.jl:66-90: expected_w = logpdf(bernoulli, false, 0.1) + logpdf(normal, 0, slope, 1)). */
gpf_status gpf_initialize_strata_proposal(gpf_handle h, const double* obs, int32_t n_obs, const double* values, int32_t n_strata, int32_t interleaved,
                                          int32_t proposal);

/* pf_resample!(state, method; priority_fn, check[, sort_particles])  src/resample.jl:19-175
 *   priority_alpha: NaN -> priority_fn = nothing; otherwise priority_fn = w -> priority_alpha * w
 *                   (the tempering family the reference's tests use, test/resample.jl:15).
 *   sort_particles: only read by GPF_RESAMPLE_STRATIFIED (src/resample.jl:143-145, default true).
 *   check:          GPF_CHECK_TRUE returns GPF_ERR_INVALID_WEIGHTS on invalid weights (src/resample.jl:55).
 *   invalid:        if non-NULL receives safe_softmax's `invalid` flag (src/utils.jl:117-140); this
 *                   synchronises the stream.  Pass NULL with check != TRUE for a fully asynchronous call.
 * Weights containing NaN/+Inf always return GPF_ERR_INVALID_WEIGHTS when checked (the reference's
 * Categorical constructor rejects NaN probabilities). */
gpf_status gpf_resample(gpf_handle h, int32_t method, double priority_alpha, int32_t sort_particles,
                        int32_t check, int32_t* invalid);

/* pf_resample!(state[1:n], method; check, sort_particles) on the WHOLE filter (or shard): the sub-state semantics of
 * src/resample.jl:185-187,205-218 -- normalised over its own n particles, log_ml_est untouched, every particle keeps
 * the log-weight logsumexp(log_weights) - log n -- without the copies a view handle makes; the gather stays deferred
 * like gpf_resample's.  On a shard of a sharded filter this is the communication-free "island" resample. */
gpf_status gpf_resample_local(gpf_handle h, int32_t method, int32_t sort_particles, int32_t check, int32_t* invalid);

/* Many small filters in one state -- the batched form of
 *     for b in blocks; if effective_sample_size(state[b]) < ess_frac * length(b); pf_resample!(state[b], method; sort_particles, check); end; end
 * (sub-states: src/view.jl:16-48, src/resample.jl:185-187,205-218; the README loop README.md:60-79 per block; the reference's own
 * tests run N = 100).  The particles are cut into consecutive blocks of block_size (the last block may be shorter).  Up to 2048 particles per
 * block ONE launch
 * resamples every block out of LDS with the sub-state semantics: normalised over the block, log_ml_est untouched, every particle of
 * a resampled block carries logsumexp(block weights) - log(block size), parents local to the block.  Block b's result is
 * bit-identical to the same call on a view of the block (gpf_view_create + gpf_resample), all blocks under the call's one epoch.
 *   priority_alpha: NaN = priority_fn nothing; else priority_fn = w -> priority_alpha * w per block (src/resample.jl:51-52): ancestors from
 *                the priorities, new weights log_ws + (logsumexp(block weights) - logsumexp(log_ws)), log_ws = lw[a] - lp[a] (:213-216).
 *   ess_frac:    >= 0: a block resamples only if its effective sample size is below ess_frac x its size (decided on the device;
 *                an invalid block -- ESS NaN -- does not);  < 0 or NaN: every block resamples.
 *   check / invalid: as gpf_resample, over all blocks; blocks with NaN / +Inf weights (and, with GPF_CHECK_TRUE, all -Inf blocks)
 *                are left as they stand, the other blocks resample, and the call returns GPF_ERR_INVALID_WEIGHTS.  (With ess_frac >= 0 an
 *                invalid block never reaches the resampler -- its ESS is NaN -- and nothing is reported, as in the loop.)
 *   n_resampled: if non-NULL receives the number of blocks that resampled (synchronises).
 * Blocks of more than 2048 particles (no size limit in the reference's loop, test/resample.jl:130-162) are resampled one after the other with the
 * full-size kernels through view handles the filter keeps -- the same results, the same single epoch, one set of launches per block.
 * Not on sharded filters, views or filters with a whole-filter trajectory store (GPF_ERR_STATE). */
gpf_status gpf_resample_blocks(gpf_handle h, int32_t method, int64_t block_size, double priority_alpha, int32_t sort_particles,
                               double ess_frac, int32_t check, int32_t* invalid, int64_t* n_resampled);
/* Conditional SMC, the resampling half: gpf_resample_blocks(method = multinomial, priority_fn nothing) in which the RETAINED particle of every
 * block -- slot 0, particle b * block_size -- survives.  This is the conditional multinomial step of Andrieu, Doucet & Holenstein (2010), "Particle
 * Markov chain Monte Carlo methods", JRSS B 72(3), section 4.3 (conditional SMC update, step (b): "sample A_{n-1}^{-B} ~ r(. | W_{n-1}, B)"); the
 * reference package has no counterpart (src/resample.jl:19-175 resamples every slot).  In every block that resamples:
 *   - slot 0's ancestor is local index 0: its row is copied from the block's own slot 0, and gpf_parents / the trajectory store record parent 0;
 *   - the slots j >= 1 get exactly the ancestors of the unconditional call: the same counters (slot b * block_size + j, the call's epoch), the
 *     same CDF over ALL particles of the block, slot 0 included;
 *   - the new weights are gpf_resample_blocks's: every particle of the block carries logsumexp(block weights) - log(block size).
 * ess_frac, check, invalid, n_resampled, the validity flags, gpf_block_resampled and the epoch advance are those of gpf_resample_blocks; the
 * block-wise trajectory store composes the recorded parents as it does there.  With gpf_{initialize,update}_blocks_ref below this is the
 * conditional filter particle Gibbs and the cSMC rejuvenation of SMC^2 run per block.
 * Refused with the state untouched, epoch included:
 *   - method GPF_RESAMPLE_RESIDUAL or _STRATIFIED (GPF_ERR_INVALID_ARGUMENT): forcing one slot is not a valid conditional scheme for them --
 *     their slots are not exchangeable, the conditional law of the other ancestors given the retained one is not their unconditional law;
 *   - there is no priority_fn argument: priorities are not offered;
 *   - blocks of more than 2048 particles (GPF_ERR_INVALID_ARGUMENT): they resample through the loop over view handles, which has no conditional form;
 *   - everything gpf_resample_blocks refuses: views, shards of a sharded filter, filters with a whole-filter trajectory store (GPF_ERR_STATE),
 *     block_size < 1, an unknown method. */
gpf_status gpf_resample_blocks_conditional(gpf_handle h, int32_t method, int64_t block_size, double ess_frac, int32_t check,
                                           int32_t* invalid, int64_t* n_resampled);
/* Particle Gibbs with ANCESTOR SAMPLING, the resampling half: gpf_resample_blocks_conditional in which the retained particle of every block that
 * resamples draws its ancestor instead of keeping itself -- Lindsten, Jordan & Schoen (2014), "Particle Gibbs with ancestor sampling", JMLR 15,
 * 2145-2184 (algorithm 2, the ancestor sampling step); the reference package has no counterpart.  Slot 0 -- particle b * block_size -- takes
 *     P(a_0 = i)  proportional to  w_{t-1}^i f(x'_t | x_{t-1}^i),
 * x'_t the block's NEXT reference value and f the model's transition density: the same target stays invariant and the retained path is broken up at
 * every step, where the plain conditional step renews its early part only when the whole genealogy coalesces away from slot 0.
 *   obs [n_blocks][n_obs], ref [n_blocks][n_ref] (host): the arguments of the gpf_update_blocks_ref that FOLLOWS -- the data vector and the reference
 *       value of the step being entered (object_motion's transition reads the step's sin(t) covariate).  They are staged into scratch of their own:
 *       the filter's per-block observations are untouched (a gpf_rejuvenate_blocks between this call and the update still sees the previous step's),
 *       no copy and no mode stay behind the call.
 *   ancestor weights  lwa_i = lw_i + logtrans(P_b, x_{t-1}^i, x'_t, obs_b), logtrans = log f minus the terms that do not depend on x_{t-1} (they
 *       cancel), P_b the block's parameter row under gpf_set_block_params, else the filter's.  Their maximum, validity flags, K-bit fixed-point weights
 *       and exact CDF are formed as for every resampler here (K from the block's particle count).
 *   the draw  a_0 = first index whose CDF exceeds mulhi64(U, S'), U the resample uniform of slot b * block_size in the call's epoch: slot 0's OWN
 *       counter, which the unconditional call uses for slot 0 and the conditional call leaves unused.
 *   fallback  ancestor weights that hold a NaN or +Inf, or are all -Inf (a reference no particle of the block can lead to, e.g. line_model with a
 *       slope no particle holds): a_0 = 0, the plain conditional step, and the call succeeds.
 * Everything else is gpf_resample_blocks_conditional's: the slots j >= 1 (same counters, same CDF of the weights), the new weights of every particle,
 * slot 0 included, ess_frac, check, invalid, n_resampled, gpf_block_resampled, the epoch advance and the trajectory store, which composes whatever
 * parent slot 0 records.  A block that does not resample draws no ancestor.  One launch.
 * Refused with the state untouched, epoch included: everything gpf_resample_blocks_conditional refuses, with its status codes; obs or ref NULL, n_obs
 * or n_ref not the model's, a non-finite value in ref (GPF_ERR_INVALID_ARGUMENT; obs as gpf_update_blocks refuses it); a block_size that differs from
 * the per-block parameters' (GPF_ERR_INVALID_ARGUMENT). */
gpf_status gpf_resample_blocks_ancestor(gpf_handle h, int32_t method, int64_t block_size, double ess_frac, int32_t check,
                                        const double* obs, int32_t n_obs, const double* ref, int32_t n_ref,
                                        int32_t* invalid, int64_t* n_resampled);
/* The ancestor weights of gpf_resample_blocks_ancestor by themselves: out[i] = lwa_i = lw_i + logtrans(P_b, x^i, ref_b, obs_b), b = i / block_size, for
 * all n particles in one launch -- what a caller needs for a backward simulation of its own, and the first half of the draw above, bit for bit.  Per
 * particle, so any block size (the parameter rows of gpf_set_block_params keep their own block size).  Reads the state and changes nothing (no epoch
 * advance, no RNG draw); synchronises the stream.  Refusals: as gpf_resample_blocks_ancestor, except the 2048-particle limit and the block size of
 * the per-block parameters; out NULL (GPF_ERR_INVALID_ARGUMENT). */
gpf_status gpf_block_ancestor_log_weights(gpf_handle h, int64_t block_size, const double* obs, int32_t n_obs,
                                          const double* ref, int32_t n_ref, double* out /* HOST [n] */);
/* which blocks the last gpf_resample_blocks resampled: out[ceil(n / block_size)] (host), 1 / 0 */
gpf_status gpf_block_resampled(gpf_handle h, int32_t* out);
/* effective_sample_size(state[b]) and log_ml_estimate(state[b]) = log_ml_est + logsumexp(block weights) - log(block size) of every block
 * (src/utils.jl:163-178); host arrays of ceil(n / block_size) doubles, either may be NULL */
gpf_status gpf_block_stats(gpf_handle h, int64_t block_size, double* ess_out, double* lml_out);
/* The state estimates of every block -- the batched form of
 *     for b in blocks; mean(state[b], addr); var(state[b], addr); proportionmap(state[b], addr); end
 * (src/statistics.jl:13-14, 48-50, 91-101 on ParticleFilterSubStates, src/view.jl:35-48).  Blocks as in gpf_resample_blocks, n_blocks =
 * ceil(n / block_size), the last block may be shorter.  Up to 2048 particles per block ONE launch answers all blocks and all columns; block b's
 * values are bit-identical to gpf_mean / gpf_var / gpf_proportion on gpf_view_create(h, b * block_size, count_b): weights normalised over the
 * block in fixed point (K from the block's particle count; 1 each if all its log-weights are -Inf), the terms summed by the binary tree of
 * DESIGN.md 3.5 over the block-local index -- a block is one 2048-term chunk of it.  Larger blocks run the loop over view handles inside
 * the library (as gpf_block_stats does): the same results, a few launches per block and column.
 * DEVIATION from the per-view calls: a block whose log-weights hold a NaN or +Inf gets NaN in all its outputs (as its ESS from
 * gpf_block_stats) and the call succeeds; the other blocks are unaffected.
 * The calls read the state and change nothing: no epoch advance, no RNG draw.  They do not read model parameters, so they work unchanged
 * with gpf_set_block_params.  Not on views, shards of a sharded filter or filters with a whole-filter trajectory store (GPF_ERR_STATE); bad arguments
 * return GPF_ERR_INVALID_ARGUMENT.  Both synchronise the stream.
 *
 * for b in blocks: [mean(state[b], c) for c in columns], [var(state[b], c) ...]   (src/statistics.jl:13-14, 48-50 on sub-states)
 * mean_out, var_out: [n_blocks][row_width] row-major, host; either may be NULL, not both.  row_width as gpf_state_dim reports it (the
 * x_{t-1} columns of keep_prev included, like gpf_mean). */
gpf_status gpf_block_moments(gpf_handle h, int64_t block_size, double* mean_out, double* var_out);
/* for b in blocks: sum of the normalised weights of block b's particles whose `column` equals values[k]   (src/statistics.jl:91-101)
 * out: [n_blocks][n_values] row-major, host; 1 <= n_values <= 16.  A value no particle of the block holds gives 0.0. */
gpf_status gpf_block_proportion(gpf_handle h, int64_t block_size, int32_t column, const double* values, int32_t n_values, double* out);

/* The other steps of the loop over sub-states, block by block in one launch each (blocks as in gpf_resample_blocks):
 *   gpf_initialize_blocks / gpf_update_blocks: block b is initialised / extended with ITS OWN observation vector
 *     (for b in blocks; pf_update!(state[b], new_args, argdiffs, observations[b]); end -- per-view updates, test/update.jl:179-189);
 *     obs = [n_blocks][n_obs] doubles (host), row b for block b.  Default proposal only.
 *   gpf_rejuvenate_blocks: pf_rejuvenate!(state[b], ...) with the block's latest observation; only_resampled != 0: only in the blocks
 *     the last gpf_resample_blocks resampled (the README loop rejuvenates inside its `if`), the others keep particles and weights.
 *     n_accepted as in gpf_rejuvenate (over the blocks that took part).
 * After gpf_update_blocks the whole-filter gpf_rejuvenate also uses the per-block observations; gpf_update / gpf_initialize go back
 * to one observation for all particles.  Each call advances the epoch once; block b's result is bit-identical to the same call on a
 * view of the block.  Not on sharded filters, views or filters with a whole-filter trajectory store. */
gpf_status gpf_initialize_blocks(gpf_handle h, const double* obs, int32_t n_obs, int64_t block_size);
gpf_status gpf_update_blocks(gpf_handle h, const double* obs, int32_t n_obs, int64_t block_size);
/* the same with a proposal PER BLOCK -- "Update with different proposals per view", test/update.jl:179-189, in one launch:
 * use_proposal[b] != 0 extends block b with the model's native proposal (src/update.jl:79-96, gpf_update_proposal's), 0 with the default
 * one (src/update.jl:12-25).  use_proposal: HOST int32[n_blocks]. */
gpf_status gpf_update_blocks_proposal(gpf_handle h, const double* obs, int32_t n_obs, int64_t block_size, const int32_t* use_proposal, int32_t proposal);
/* stratified initialisation / update of every block by itself (src/initialize.jl:92-109, src/update.jl:193-210 on each sub-state, one launch):
 * a particle's stratum follows from its index INSIDE its block and the block's own particle count (stratified_map!, src/utils.jl:29-55);
 * values / n_strata / interleaved as in gpf_initialize_strata, the same strata for all blocks */
gpf_status gpf_initialize_blocks_strata(gpf_handle h, const double* obs, int32_t n_obs, int64_t block_size, const double* values, int32_t n_strata, int32_t interleaved);
gpf_status gpf_update_blocks_strata(gpf_handle h, const double* obs, int32_t n_obs, int64_t block_size, const double* values, int32_t n_strata, int32_t interleaved);
gpf_status gpf_rejuvenate_blocks(gpf_handle h, int32_t method, int32_t n_iters, int32_t only_resampled, uint64_t* n_accepted);
/* A whole series per block in ONE launch: the filter loop of README.md:60-79 run per block (the block-wise resampling of test/resample.jl:130-162
 * followed by the per-view update),
 *     for t in 1:n_steps
 *         gpf_resample_blocks(h, method, block_size, NaN, sort_particles, ess_frac, GPF_CHECK_FALSE, NULL, NULL);      epoch E + 2(t-1)
 *         gpf_update_blocks(h, obs[:, t], n_obs, block_size);                                                          epoch E + 2(t-1) + 1
 *     end
 * for the callers that filter y_1:T again and again under new parameters (SMC^2 rejuvenation, parallel particle-marginal MH, a likelihood surface over
 * a theta grid: gpf_set_block_params, gpf_resample_across_blocks, gpf_block_stats).  The blocks do not interact inside this loop, so one team -- a wave
 * up to 512 particles per block, a workgroup up to 2048 -- runs all steps of its block with no launch in between.
 *   contract  on an initialised filter at epoch E the call leaves EXACTLY what the loop leaves after n_steps iterations: rows, log-weights, parents
 *             (block-local, written only when a block resamples, the last write stands), the epoch E + 2 n_steps, the per-block observation rows of
 *             the last step, the block size, "no gpf_resample_blocks to refer to" (gpf_block_resampled, only_resampled) -- bit for bit, so every
 *             later call continues identically and two calls of T1 and T2 steps equal one of T1 + T2.  Resample slot gid0 + b block_size + j draws
 *             under epoch E + 2(t-1), the propagate of particle gid under E + 2(t-1) + 1, exactly as the two calls do.  Per-block parameters
 *             (gpf_set_block_params) are used as gpf_update_blocks uses them.
 *   obs       HOST, [n_blocks][n_steps][n_obs]: block b's series, step-major inside the block; shared_obs != 0: [n_steps][n_obs], ONE series for all
 *             blocks.  All values finite, n_obs the model's.  Copied to the device once per call.
 *   outputs   HOST, each may be NULL: ess_out, lml_out [n_steps][n_blocks] -- what gpf_block_stats returns after step t's update, bit for bit;
 *             resampled_out [n_steps][n_blocks] -- the word of step t's resample: bit 0 = the block resampled (gpf_block_resampled), bits 8.. = the
 *             validity flags it reported (1 NaN, 2 +Inf, 4 all -Inf); *invalid = 1 if any flag was reported at any step.
 *   ess_frac  as in gpf_resample_blocks; NaN: every block resamples at every step.
 *   weights   a block whose weights hold a NaN or +Inf is skipped by the resample and propagated anyway, at every step; after the whole run the call
 *             returns GPF_ERR_INVALID_WEIGHTS ("Invalid weights (NaN)."), the state being what the loop leaves when every iteration's error is
 *             ignored.  An all -Inf block resamples with uniform weights where its gate lets it (safe_softmax's fallback) and sets *invalid.
 *   timing    the launch is booked under GPF_K_STEP (gpf_kernel_timing).
 *   refused   nothing changed, epoch included.  GPF_ERR_STATE: a sub-state view, a shard, a trajectory store of either kind (recording a step is host
 *             bookkeeping per step), forward smoothing per block, a keep_prev filter (x_{t-1} serves only the moves), strata set on the filter;
 *             GPF_ERR_INVALID_ARGUMENT: block_size < 1, a clamped block_size > 2048 or other than the per-block parameters', n_steps < 1 or > 4096
 *             (chunks compose), more than 2^31 observation words on the device, obs NULL, n_obs not the model's, a non-finite observation;
 *             GPF_ERR_UNKNOWN_METHOD.  Not offered inside the run (the loop of calls has them): rejuvenation, proposals, a reference path, tempering,
 *             the initial step (gpf_initialize_blocks stays a call of its own). */
gpf_status gpf_run_blocks(gpf_handle h, const double* obs, int32_t n_obs, int32_t n_steps, int32_t shared_obs,
                          int64_t block_size, int32_t method, int32_t sort_particles, double ess_frac,
                          double* ess_out, double* lml_out, int32_t* resampled_out, int32_t* invalid);
/* Conditional SMC, the propagation half: gpf_initialize_blocks / gpf_update_blocks with ONE PARTICLE PER BLOCK PINNED to a given value -- the
 * conditional filter of Andrieu, Doucet & Holenstein (2010), section 4.3 (step (a) / (b): "set X_n^{B_n} = the retained path, sample the other
 * N - 1 particles"), on the reference's per-view loop
 *     for b in blocks; pf_update!(state[b], new_args, argdiffs, observations[b]); end      (test/update.jl:179-189; src/update.jl:12-25)
 * of which the reference itself has no conditional form.
 *   ref: HOST [n_blocks][n_ref] doubles, row b for block b, n_ref = the model's dimension (its latent columns); a per-call input: the library
 *        keeps no "conditional mode" and no copy of the reference between calls.
 * Slot 0 of block b is particle b * block_size.  Its latent columns become ref[b] instead of the model's draw; its weight increment is
 * log p(y_b | ref[b]) under the block's parameters -- the bootstrap weight, no transition density is needed; on an update lw' = lw + that
 * increment with the incoming lw, and with keep_prev the x_{t-1} columns are the incoming row's latent columns, as for any particle; every other
 * column is 0.  Every other particle is bit-identical to the same call without a reference on the same incoming state (counter-based RNG: slot
 * 0's unused counters disturb nobody).  Epoch advance, per-block observations, the tracked maximum and flags and the trajectory store's snapshot
 * behave as in the plain call; the store records the pinned value.  Works with and without gpf_set_block_params and keep_prev, for any block size.
 * The values of DISCRETE latents in ref (the moving / slope / outlier indicators of the models that have one) are the caller's business: they are
 * stored as given.  Rejuvenation is not restricted: a move on slot 0 changes the retained value at the current step.
 * Refused with nothing changed (no store, launch, epoch advance or trajectory-store step), GPF_ERR_INVALID_ARGUMENT:
 *   - ref NULL, n_ref other than the model's dimension, any value of ref not finite (NaN, +-Inf);
 *   - everything the plain calls refuse (their status codes).
 * Pinning is offered with the default proposal only: the strata, per-block-proposal and native-proposal forms take no reference. */
gpf_status gpf_initialize_blocks_ref(gpf_handle h, const double* obs, int32_t n_obs, int64_t block_size, const double* ref, int32_t n_ref);
gpf_status gpf_update_blocks_ref(gpf_handle h, const double* obs, int32_t n_obs, int64_t block_size, const double* ref, int32_t n_ref);
/* for b in blocks: the model arguments of state[b] (src/update.jl:12-25 on a sub-state with new_args_b) -- many parameter values in one state,
 * e.g. the likelihood p(y_1:T | theta_b) of every block from gpf_block_stats.
 *   params: HOST [n_blocks][n_params] doubles, row b = block b's parameter vector in the layout of csrc/gpf_models.hpp (derived constants
 *           included, exactly as gpf_config.params); 1 <= n_params <= 24; NULL clears them (n_params and block_size are then ignored).
 *   block_size: as in the block-wise calls (clamped to the particle count); n_blocks = ceil(n / block_size).
 * The rows are uploaded once and stay in force until they are cleared or the handle is destroyed.  While they are set:
 *   - every block-wise step uses row b for block b: gpf_initialize_blocks, gpf_update_blocks, gpf_update_blocks_proposal,
 *     gpf_{initialize,update}_blocks_strata and gpf_rejuvenate_blocks (move and reweight), and the whole-filter gpf_rejuvenate when it
 *     delegates to gpf_rejuvenate_blocks after a block-wise update.  Block b's rows, weights, parents, accept counts and gpf_block_stats
 *     entries are bit-identical to those of block b of the same calls on a filter created with params = row b (same seed, epochs and
 *     particle ids: the RNG counters do not depend on the parameters);
 *   - a block-wise step whose (clamped) block_size differs from the rows' returns GPF_ERR_INVALID_ARGUMENT and changes nothing;
 *   - every call that would use gpf_config.params returns GPF_ERR_STATE and changes nothing: gpf_initialize*, gpf_update*, gpf_step_ess,
 *     gpf_introduce, gpf_rejuvenate* other than the delegation above, any of these on a view of the filter, and the resize family
 *     (gpf_resize, gpf_replicate, gpf_dereplicate, gpf_coalesce), which would break the block layout;
 *   - model-independent calls work as before: gpf_resample*, gpf_resample_blocks, gpf_block_stats, the getters, views, checkpoints.
 * Clearing the rows restores the behaviour without them exactly.  A checkpoint does not hold the rows (the blob layout is unchanged) and
 * gpf_checkpoint_load neither sets nor clears them: restore, then call gpf_set_block_params again to continue bit for bit.
 * Not on views, shards of a sharded filter or filters with a whole-filter trajectory store (GPF_ERR_STATE); a NULL handle, n_params outside 1..24 or
 * block_size < 1 return GPF_ERR_INVALID_ARGUMENT and change nothing. */
gpf_status gpf_set_block_params(gpf_handle h, const double* params, int32_t n_params, int64_t block_size);
/* the per-block parameter rows as they stand: out = HOST [n_blocks][n_params] doubles, the first n_params entries of every row (n_blocks must be
 * the rows' block count).  After gpf_resample_across_blocks the rows are permuted by its block ancestors; a checkpoint does not hold them, so
 * this getter (or gpf_block_ancestors) is how a caller keeps track of them.  GPF_ERR_STATE when none are set. */
gpf_status gpf_get_block_params(gpf_handle h, double* out, int32_t n_params, int64_t n_blocks);

/* Resampling ACROSS blocks -- the outer level of SMC^2, a nested or an island particle filter: every block is one "super-particle" whose weight is
 * its likelihood estimate, blocks are resampled and whole filters are copied.  It is the reference's resampler (src/resample.jl:19-175) applied one
 * level up, to B = n / block_size consecutive, congruent blocks:
 *   1. L[b] = log_ml_estimate(state[b]) = log_ml_est + logsumexp(block b) - log(block_size): exactly the double gpf_block_stats reports.
 *   2. the planner: a filter of B particles with the handle's seed, gid0 = 0, log_ml_est = 0, log-weights L and the handle's RNG epoch E at the call.
 *        ess = effective_sample_size(planner)   (-> *ess_out),      M = log_ml_estimate(planner) = logsumexp(L) - log B,
 *        A[0..B) = the ancestors gpf_resample(planner, method, NaN, sort_particles) yields: bit-identical to a stand-alone filter of B particles.
 *      method: GPF_RESAMPLE_MULTINOMIAL | _RESIDUAL | _STRATIFIED (else GPF_ERR_UNKNOWN_METHOD).
 *   3. ess_frac >= 0: resample only if ess < ess_frac x B (decided on the host: the caller needs the verdict to jitter its parameters);
 *      ess_frac < 0 or NaN: always.  *resampled = 1 / 0.  A call whose gate does not fire changes nothing but the epoch.
 *   4. when it fires, the new block b is a complete copy of the old block a = A[b], for i < block_size:
 *        rows'[b bs + i] = rows[a bs + i] (the full row, keep_prev columns included),       parents'[b bs + i] = a bs + i + 1,
 *        lw'[b bs + i]   = lw[a bs + i] + delta_a,   delta_a = M - L[a] in double (0 where L[a] = -Inf),
 *      the per-block parameter rows (gpf_set_block_params) and, after a block-wise update, the per-block observations: row b' = old row A[b].
 *      Every block's gpf_block_stats estimate then equals M up to rounding; log_ml_est is untouched (the sub-state rule, src/resample.jl:185-187,
 *      205-218, one level up).
 *      DEVIATION from pf_resample! on a sub-state: the weights INSIDE a block are not reset -- its inner filter carries on, only its total
 *      mass becomes the average mass.
 *   5. the RNG epoch advances once per accepted call, fired or not (as gpf_resample_blocks).  A call that fired invalidates the "resampled last"
 *      mask of gpf_resample_blocks (gpf_rejuvenate_blocks(only_resampled) then fails) and the cached weight summaries, also those of views.  A
 *      deferred gather or lazy move is materialised first.
 *   6. a NaN or +Inf L[b] (a block with NaN / +Inf weights): GPF_ERR_INVALID_WEIGHTS, state and epoch untouched, *invalid = 1, whatever `check`
 *      says.  All L = -Inf: with GPF_CHECK_TRUE the same refusal; else safe_softmax's uniform fallback as in gpf_resample (ancestors from
 *      uniform block weights, every delta = 0, *invalid = 1; its ESS is NaN, so a gated call does not fire).
 * Refused without changing anything: n not a multiple of block_size, block_size < 1, a block_size other than that of the per-block parameters or
 * of the per-block observations (GPF_ERR_INVALID_ARGUMENT); views, shards of a sharded filter, filters with a whole-filter trajectory store (GPF_ERR_STATE).
 * B = 1 is legal: A = [0], delta = 0, the state comes back bit for bit.  Blocks of any size (no LDS limit); beyond 2048 particles per block L comes
 * from gpf_block_stats's loop over view handles.  Not here: priorities / tempering at block level, sharded filters, parameter jitter (host:
 * theta = theta[A], perturb, gpf_set_block_params).  invalid / resampled / ess_out may be NULL. */
gpf_status gpf_resample_across_blocks(gpf_handle h, int32_t method, int64_t block_size, int32_t sort_particles, double ess_frac, int32_t check,
                                      int32_t* invalid, int32_t* resampled, double* ess_out);
/* the 1-based block ancestors A of the last gpf_resample_across_blocks that fired: out = HOST int64[B].  GPF_ERR_STATE before any such call and
 * after a resize or a re-initialisation. */
gpf_status gpf_block_ancestors(gpf_handle h, int64_t* out);

/* same, with log_priorities = priority_fn.(log_weights) evaluated by the caller (any closure):
 * log_priorities is a HOST array of n_particles doubles. */
gpf_status gpf_resample_with_priorities(gpf_handle h, int32_t method, const double* log_priorities,
                                        int32_t sort_particles, int32_t check, int32_t* invalid);

/* pf_rejuvenate!(state, kern, kern_args, n_iters; method)          src/rejuvenate.jl:18-90
 * native kernels: GPF_REJUVENATE_MOVE     = pf_move_accept!  with kern = Gen.mh(trace, select(current step))
 *                 GPF_REJUVENATE_REWEIGHT = pf_move_reweight! with kern = move_reweight(trace, selection)
 *                                           (src/rejuvenate.jl:125-132)
 * n_accepted (may be NULL; non-NULL synchronises) replaces the per-particle @debug log
 * (src/rejuvenate.jl:47). Requires keep_prev = 1. */
gpf_status gpf_rejuvenate(gpf_handle h, int32_t method, int32_t n_iters, uint64_t* n_accepted);

/* pf_move_reweight!(state, move_reweight, (proposal, proposal_args), n_iters)   src/rejuvenate.jl:74-90 with the PROPOSAL variant
 * of the kernel, move_reweight(trace, proposal, proposal_args) (src/rejuvenate.jl:134-148): the current step's latent is proposed by a
 * NATIVE proposal q, the trace is updated with it, log_weights[i] += weight - fwd_score + bwd_score.
 *   GPF_MOVE_PROPOSAL_LOCALLY_OPTIMAL  (GPF_MODEL_LGSSM2, no parameters): q = p(x_t | x_{t-1}, y_t) -- a Gibbs move, relative weight 0 up to rounding
 *   GPF_MOVE_PROPOSAL_LINE_OUTLIER     (GPF_MODEL_LINE, params = {q, log q, log(1 - q)}): {:line => t => :outlier} ~ bernoulli(q), the
 *                                      outlier_propose of the reference's test (test/rejuvenate.jl:19-27, q = 0.9)
 * Requires keep_prev = 1 like gpf_rejuvenate. */
typedef enum { GPF_MOVE_PROPOSAL_LOCALLY_OPTIMAL = 1, GPF_MOVE_PROPOSAL_LINE_OUTLIER = 2 } gpf_move_proposal;
gpf_status gpf_rejuvenate_proposal(gpf_handle h, int32_t proposal, const double* params, int32_t n_params, int32_t n_iters);
/* the same native proposals under either rejuvenation method (method::Symbol of pf_rejuvenate!, src/rejuvenate.jl:18-27):
 * GPF_REJUVENATE_REWEIGHT = gpf_rejuvenate_proposal above; GPF_REJUVENATE_MOVE = pf_move_accept!(state, mh, (proposal, proposal_args), n_iters)
 * (src/rejuvenate.jl:40-53 with Gen.mh(trace, proposal, proposal_args)): propose, update, assess the reverse move, accept iff
 * log(rand()) < weight - fwd_score + bwd_score; the weights stay.  n_accepted (may be NULL): accepted proposals over all particles and sweeps. */
gpf_status gpf_rejuvenate_with_proposal(gpf_handle h, int32_t method, int32_t proposal, const double* params, int32_t n_params, int32_t n_iters,
                                        uint64_t* n_accepted);

/* "Lazy search" (csrc/gpf_k_fused.hpp): with enable != 0 a plain pf_resample!(state, :multinomial) enqueues the weight scan
 * only and the pf_update! that follows finds the ancestors, gathers, propagates and writes state.parents in ONE kernel; any other consumer
 * runs the stand-alone search first.  Same results bit for bit.  OFF by default (GPF_LAZY_SEARCH=1 in the environment turns it on for new
 * handles): measured on MI355X it is no faster than the two kernels (profiles/r04_lazy_search.txt). */
gpf_status gpf_set_lazy_search(gpf_handle h, int32_t enable);

/* ---- weight summaries ---------------------------------------------------------------------- */
/* effective_sample_size(state) / get_ess                            src/utils.jl:163-164,171 */
gpf_status gpf_effective_sample_size(gpf_handle h, double* out);
/* Gen.log_ml_estimate(state) / get_lml_est                          src/utils.jl:186 */
gpf_status gpf_log_ml_estimate(gpf_handle h, double* out);
/* Gen.get_log_weights(state) */
gpf_status gpf_get_log_weights(gpf_handle h, double* out, int64_t n);
/* get_log_norm_weights(state)                                       src/utils.jl:148 */
gpf_status gpf_get_log_norm_weights(gpf_handle h, double* out, int64_t n);
/* get_norm_weights(state)                                           src/utils.jl:156 */
gpf_status gpf_get_norm_weights(gpf_handle h, double* out, int64_t n);
/* state.parents (1-based, global)                                   test/resample.jl:11 */
gpf_status gpf_get_parents(gpf_handle h, int64_t* out, int64_t n);

/* ---- state access (Gen.get_traces: one latent address = one column) ------------------------- */
gpf_status gpf_state_dim(gpf_handle h, int32_t* dim, int32_t* row_width);
gpf_status gpf_get_column(gpf_handle h, int32_t column, double* out, int64_t n);
gpf_status gpf_get_rows(gpf_handle h, double* out, int64_t n_doubles);          /* n_particles * row_width */
gpf_status gpf_set_rows(gpf_handle h, const double* rows, int64_t n_doubles);   /* ParticleFilterState(trs, ws), src/initialize.jl:8-10 */
gpf_status gpf_set_log_weights(gpf_handle h, const double* lw, int64_t n);

/* Gen.sample_unweighted_traces(state, n_samples)                    src/utils.jl:7,189-194
 * n_samples i.i.d. draws from the normalised weights; the filter is not modified.  rows_out: HOST [n_samples][row_width];
 * idx_out (may be NULL): HOST 1-based indices of the drawn particles. */
gpf_status gpf_sample_unweighted(gpf_handle h, int64_t n_samples, double* rows_out, int64_t* idx_out);

/* ---- statistics ---------------------------------------------------------------------------- */
/* mean(state, addr)                                                 src/statistics.jl:13-14 */
gpf_status gpf_mean(gpf_handle h, int32_t column, double* out);
/* var(state, addr)  (population form)                               src/statistics.jl:48-50 */
gpf_status gpf_var(gpf_handle h, int32_t column, double* out);

/* ---- measurement hooks (bench.py) ----------------------------------------------------------- */
/* kernel ids for gpf_kernel_time */
typedef enum { GPF_K_STEP = 0, GPF_K_MAX = 1, GPF_K_SCAN = 2, GPF_K_SEARCH = 3, GPF_K_GATHER = 4,
               GPF_K_MOVE = 5, GPF_K_COUNT = 6 } gpf_kernel_id;
/* enable!=0: bracket every launch of kernel `id` with hipEvents on the handle's stream */
gpf_status gpf_kernel_timing(gpf_handle h, int32_t id, int32_t enable);
/* synchronises; total elapsed milliseconds and number of launches since timing was enabled */
gpf_status gpf_kernel_time(gpf_handle h, int32_t id, double* total_ms, int64_t* launches);

/* device-side math spec, for the bitwise host/device parity tests (tests/test_math_parity.py):
 * which: 0 exp, 1 log, 2 sincos2pi (out=sin,out2=cos), 3 atan2(a,b), 4 sqrt, 5 a/b,
 *        6 normal2 from counters (a=gid as double, b=blk as double; seed/epoch/tag via the handle),
 *        7 the spacing logarithm of GPF_RESAMPLE_MULTINOMIAL_SORTED: -log((k + 1/2) 2^-52), k = the top 52 bits of a's BIT PATTERN */
gpf_status gpf_debug_math(gpf_handle h, int32_t which, const double* a, const double* b, int64_t n,
                          double* out, double* out2);

/* ---- sub-state views (src/view.jl:16-48) -----------------------------------------------------
 * state[idxs] / view(state, idxs) for a contiguous range: a handle that ALIASES particles [start, start+count) of
 * `parent` (their rows, log-weights and parents) and owns only its scratch.  Every gpf_* operation works on it with the
 * sub-state semantics of the reference: pf_update!/pf_rejuvenate! touch only the range (update_refs! copies back,
 * src/utils.jl:17-20); pf_resample! resamples inside the range with LOCAL ancestor indices, leaves the log-ML estimate
 * alone and resets the weights to the block's average so its total mass is preserved (src/resample.jl:185-187,205-218);
 * gpf_log_ml_estimate = source.log_ml_est + logsumexp(view) - log n (src/utils.jl:174-178).  RNG counters keep the
 * global particle ids.  Destroy with gpf_destroy; a view becomes stale when the parent is resized or re-initialised.
 * A view of a SHARD handle is allowed: resampling it is the communication-free local ("island") resample of that shard.
 * A filter with a trajectory store (gpf_history_enable) has no views (GPF_ERR_STATE): the store keeps one ancestor map and one
 * set of columns per time step for the WHOLE filter. */
gpf_status gpf_view_create(gpf_handle parent, int64_t start, int64_t count, gpf_handle* out);
/* state[start:step:stop] (src/view.jl:35-48 takes any AbstractVector; the reference's tests use strided ranges, state[k:5:100] and
 * state[k:2:100], test/initialize.jl:60,85, test/update.jl:33,61, test/resize.jl:138): the view's particle i is particle
 * start + i * step of `parent` (0-based start, count particles).  Same semantics as gpf_view_create; per-particle RNG counters
 * stay the parent's particle ids, the view's resample stream is indexed by the slot ids start, start + 1, ... whatever the step.
 * A strided view works on a compact copy (gathered on entry, scattered back by every mutating call: update_refs! for sub-states
 * copies back as well, src/utils.jl:17-20). */
gpf_status gpf_view_create_strided(gpf_handle parent, int64_t start, int64_t step, int64_t count, gpf_handle* out);
/* state[idxs] / view(state, idxs) for ANY vector of distinct indices (src/view.jl:35-48: `idxs::AbstractVector`): index = HOST array of
 * count 0-based particle indices of `parent`, in the order the view presents them.  Same semantics and the same compact-copy mechanism as
 * the strided view; a particle keeps its own id as its RNG counter, the view's resample stream is indexed by the slot ids index[0],
 * index[0] + 1, ...  Repeated indices are refused (GPF_ERR_INVALID_ARGUMENT): a particle written through two slots has no defined value. */
gpf_status gpf_view_create_indexed(gpf_handle parent, const int64_t* index, int64_t count, gpf_handle* out);

/* ---- resize family (src/resize.jl) --------------------------------------------------
 * The handle stays valid; its per-particle buffers are reallocated for the new count.  Unsharded filters only. */
gpf_status gpf_n_particles(gpf_handle h, int64_t* out);
/* pf_resize!(state, n_particles, method; priority_fn, check)          src/resize.jl:16-124
 * method = GPF_RESAMPLE_MULTINOMIAL | GPF_RESAMPLE_RESIDUAL | GPF_RESAMPLE_OPTIMAL;
 * priority_alpha / check / invalid as in gpf_resample.
 * GPF_RESAMPLE_OPTIMAL = pf_optimal_resize! (src/resize.jl:149-219, Fearnhead & Clifford): needs n_particles <= current
 * count, ignores priority_alpha (the reference takes no priority_fn there); particles with c w_i >= 1 are kept with
 * their weights, the rest are resampled by systematic sampling (one uniform) and share logsumexp - log c; the
 * log-ML estimate is not touched. */
gpf_status gpf_resize(gpf_handle h, int64_t n_particles, int32_t method, double priority_alpha, int32_t check, int32_t* invalid);
/* pf_replicate!(state, n_replicates; layout)                           src/resize.jl:236-244 */
gpf_status gpf_replicate(gpf_handle h, int32_t n_replicates, int32_t interleaved);
/* pf_dereplicate!(state, n_replicates; layout, method)                 src/resize.jl:267-297  (sample=0 :keepfirst, 1 :sample) */
gpf_status gpf_dereplicate(gpf_handle h, int32_t n_replicates, int32_t interleaved, int32_t sample);
/* pf_coalesce!(state; by)                                               src/resize.jl:309-334
 * Groups the particles whose key columns are equal BITWISE (Julia's isequal on Float64 apart from NaN payloads: -0.0 != 0.0) and
 * replaces every group by its first member.  key_mask: bit c = column c of the row (gpf_get_rows) is part of the key; 0 = every
 * state column -- the d latent columns, plus the d previous-state columns with keep_prev (by = get_choices / identity).  The
 * padding column of odd widths is never part of the key; a bit beyond the state columns is GPF_ERR_INVALID_ARGUMENT.
 *   row of group g       = the row of its first member;  parents[g] = that member's index + 1
 *   lw[g]                = lse_g + (log(n_new) - log(n_old)),  lse_g = lse_from(m_g, S_g, K, flags_g): m_g the group's maximum,
 *                          K = fix_K(n_old), S_g = sum of exp_fix(w_i - m_g, K) as an exact u64 sum, flags_g = ALL_NEGINF iff m_g = -Inf
 *                          (the fixed-point logsumexp of the summaries; log = the library's log, gpf_host_log)
 *   *n_out               = n_new, the number of groups (may be NULL)
 * log_ml_est, the RNG epoch and everything else are unchanged; all rows distinct: n_new = n_old and the state comes back bit for bit
 * (m + log(1.0) + 0.0; parents 1:n).  Views of the filter become stale (not when the call is refused).  Refused (GPF_ERR_STATE) on
 * sharded filters, views and filters with a trajectory store.  Device scratch of about 20 B x 2n + 4 B x n (a hash table of 2^k >= 2n
 * slots) is allocated by the call and freed before it returns; nothing stays on the handle.
 * Deviations from the reference:
 *   - order: the reference emits groups in Dict iteration order (unspecified); here in ASCENDING ORDER OF FIRST OCCURRENCE, so parents
 *     is strictly increasing and the result does not depend on the thread schedule.
 *   - sum: the reference's unshifted sum of exp(w) underflows to -Inf below about -745; the shifted fixed-point sum does not.  Because
 *     it is an integer sum, the result does not depend on summation order (device atomics are bit-reproducible).
 *   - a NaN or +Inf weight anywhere returns GPF_ERR_INVALID_WEIGHTS and leaves the state and its views untouched (the reference
 *     propagates NaN).
 *   - `by` is a set of current-step columns; closures and past-step addresses have no native form. */
gpf_status gpf_coalesce(gpf_handle h, uint64_t key_mask, int64_t* n_out);
/* pf_introduce!(state, [model, model_args,] observations, [proposal, proposal_args,] n_particles)   src/resize.jl:351-421
 * obs = [n_steps][n_obs] row-major: the per-step data vectors of steps 1..t (t = n_steps >= 1) that the reference's choicemap
 * constrains, e.g. line_choicemap(10).  Appends n_particles new particles generated over the whole history in ONE launch:
 *   new particle j = particle j of gpf_initialize's kernel at step 1 followed by t - 1 propagates from the prior (gpf_update), with
 *   RNG counter n_old + j, epochs 0 .. t-1 and the seed s' = mix(cfg.seed, epoch at the call); weight = the sum of the step
 *   log-likelihoods in step order.  proposal = GPF_PROPOSAL_* (0: none): the native proposal of the LAST step
 *   (gpf_initialize_proposal's when t = 1, else gpf_update_proposal's), earlier steps from the prior.
 *   mix(s, e): z = s ^ (e * 0x9e3779b97f4a7c15 + 0xd1b54a32d192ed03); z = (z ^ z >> 30) * 0xbf58476d1ce4e5b9;
 *              z = (z ^ z >> 27) * 0x94d049bb133111eb; mix = z ^ z >> 31   (64-bit wrap-around arithmetic)
 * The existing particles: lw += log_ml_est where log_ml_est != 0 (on the device), then log_ml_est = 0; their parents are kept; the new
 * particles' parents read 0 (no ancestor; no kernel gathers through them: the pending-resample flags are cleared with the count).  Then
 * n = n_old + n_particles and epoch += 1.  Views become stale; the same refusals as gpf_coalesce.  The reference leaves the new parents
 * undefined; the model / model_args of the reference's signature are the handle's own (checked by the bindings). */
gpf_status gpf_introduce(gpf_handle h, const double* obs, int32_t n_obs, int32_t n_steps, int64_t n_particles, int32_t proposal);

/* ---- trajectory store ------------------------------------------------------------------
 * Gen traces are persistent, so the reference can ask for a PAST choice of every surviving particle:
 * mean(state, 5 => :moving) (reference README.md:97-104, src/statistics.jl:13-14 with a past address).
 * With the store enabled the handle keeps, per time step, the step's latent columns and the composed ancestor map
 * of the resamples of that step (8d + 4 bytes per particle and step); queries follow the ancestry of each
 * current particle.  `step` is 1-based (step 1 = gpf_initialize).  Unsharded filters only. */
gpf_status gpf_history_enable(gpf_handle h, int32_t max_steps);          /* before gpf_initialize */
gpf_status gpf_history_steps(gpf_handle h, int32_t* n_steps);
gpf_status gpf_history_column(gpf_handle h, int32_t step, int32_t column, double* out, int64_t n);   /* trace[step => column] per particle */
gpf_status gpf_history_mean(gpf_handle h, int32_t step, int32_t column, double* out);               /* mean(state, step => column) */
gpf_status gpf_history_var(gpf_handle h, int32_t step, int32_t column, double* out);                /* var(state, step => column)  */
/* proportionmap(state, addr)[value]  (src/statistics.jl:91-101): normalised weight of the particles whose column == value;
 * step = 0 -> current step's column, step >= 1 -> past choice (trajectory store) */
gpf_status gpf_proportion(gpf_handle h, int32_t step, int32_t column, double value, double* out);

/* ---- the block-wise trajectory store: past choices per block ------------------------------------------------
 * A sub-state is a slice of persistent traces (src/view.jl:35-48), so the reference answers mean(state[b], 5 => :moving) for any block of
 * "many small filters in one state".  gpf_history_enable_blocks is gpf_history_enable -- same preconditions (before initialisation, unsharded,
 * max_steps >= 1), same store, same whole-filter calls and queries (gpf_update, gpf_resample, gpf_rejuvenate, gpf_history_*, gpf_proportion) --
 * and declares that the block-wise calls feed the store too; a store enabled with gpf_history_enable keeps refusing them (GPF_ERR_STATE).
 *   recording: gpf_initialize_blocks* begins step 1, gpf_update_blocks* begins the next step (a full store returns GPF_ERR_STATE and leaves rows,
 *     weights, per-block observations and the epoch untouched; so does a call refused for its observations: it begins no step and an
 *     initialisation so refused clears nothing); gpf_rejuvenate_blocks is seen when the step ends or at query time;
 *     gpf_resample_blocks composes, for the blocks that resampled, their block-local parents into the step's ancestor map (the particles of the
 *     other blocks stay where they are); gpf_resample_across_blocks composes its global parents when it fires, nothing when it does not.
 *     Several resamples of one step compose in call order (a nested filter: gpf_resample_blocks, then gpf_resample_across_blocks).
 *   blocks of more than 2048 particles are the work of view handles inside the library and a filter with a store has no views: with a (clamped)
 *     block_size > 2048, gpf_resample_blocks, gpf_block_stats, gpf_block_moments, gpf_block_proportion, gpf_resample_across_blocks and the two
 *     queries below return GPF_ERR_STATE and change nothing.  gpf_initialize_blocks*, gpf_update_blocks* and gpf_rejuvenate_blocks take any size.
 *   still refused on either store: views, gpf_resize / gpf_coalesce / gpf_introduce, gpf_checkpoint_load.
 *
 * The queries -- the batched form of
 *     for b in blocks; mean(state[b], step => addr); var(state[b], step => addr); proportionmap(state[b], step => addr); end
 * (src/statistics.jl:13-14, 48-50, 91-101 on ParticleFilterSubStates, src/view.jl:35-48) -- answer all blocks and all latent columns in ONE launch.
 * step is 1-based, 1 <= step <= gpf_history_steps; blocks as in gpf_block_moments (n_blocks = ceil(n / block_size), the last may be shorter).
 * Every particle's value is trace[step => column] along its ancestry (what gpf_history_column returns); the weights are the block's CURRENT
 * log-weights, normalised and summed exactly as gpf_block_moments / gpf_block_proportion do (the tree of DESIGN.md 3.5 over the block-local index):
 * the results are bit-identical to those calls on a filter of the same log-weights whose rows hold the past values.
 * DEVIATION, as in gpf_block_moments: a block whose log-weights hold a NaN or +Inf reads NaN and the call succeeds; the other blocks are unaffected.
 * The queries read the state and change nothing (no epoch advance, no RNG draw) and synchronise the stream.  Without a block-wise store:
 * GPF_ERR_STATE; bad step / column / n_values / NULL arguments: GPF_ERR_INVALID_ARGUMENT, nothing is written.
 *
 * mean_out, var_out: [n_blocks][dim] row-major, host, dim as gpf_state_dim reports it (the store keeps the latent columns, not the row width);
 * either may be NULL, not both. */
gpf_status gpf_history_enable_blocks(gpf_handle h, int32_t max_steps);   /* before gpf_initialize_blocks / gpf_initialize */
gpf_status gpf_block_history_moments(gpf_handle h, int32_t step, int64_t block_size, double* mean_out, double* var_out);
/* out: [n_blocks][n_values] row-major, host; 1 <= n_values <= 16, 0 <= column < dim.  A value no particle of the block held gives 0.0. */
gpf_status gpf_block_history_proportion(gpf_handle h, int32_t step, int64_t block_size, int32_t column, const double* values, int32_t n_values, double* out);
/* Whole trajectories per block: the batched form of
 *     for b in blocks; sample_unweighted_traces(state[b], n_samples); end
 * (Gen.sample_unweighted_traces, src/utils.jl:7,189-194 on a ParticleFilterSubState, src/view.jl:35-48).  The reference's traces are persistent, so
 * every draw is a whole path x_1:T of block b: what SMC^2 / particle marginal MH keep per theta, what particle Gibbs conditions its next sweep
 * on, what a nested filter reports per island.  ONE launch does the weights, the draws, the genealogy walk and the gather of all blocks.
 *   blocks    as in gpf_block_moments: block_size is clamped to the particle count, n_blocks = ceil(n / block_size), the last block may be shorter.
 *             Needs the block-wise store (without it: GPF_ERR_STATE naming the trajectory store); a clamped block_size > 2048 is refused with
 *             GPF_ERR_STATE like the other block queries on a store (it would need sub-state views, which a filter with a store does not have).
 *   steps     step_lo, step_hi: 1-based and inclusive, 1 <= step_lo <= step_hi <= gpf_history_steps; n_steps = step_hi - step_lo + 1.
 *   traj_out  HOST [n_blocks][n_samples][n_steps][dim] row-major, dim as gpf_state_dim reports it; idx_out: HOST int64 [n_blocks][n_samples], the
 *             1-based index INSIDE the block of the drawn current particle.  Either may be NULL, not both.
 *   refused   with GPF_ERR_INVALID_ARGUMENT, nothing written: n_samples < 1, n_blocks * n_samples >= 2^31, n_blocks * n_samples * n_steps * dim
 *             >= 2^31, bad steps, both outputs NULL, block_size < 1, a NULL handle.
 * The draw: for block b of cnt particles K = fix_K(cnt); maximum and flags as in safe_softmax (src/utils.jl:117-140);
 * q_i = exp_fix(lw_i - m, K), every q_i = 1 if all log-weights of the block are -Inf (the uniform fallback, as in gpf_sample_unweighted); cdf = the
 * inclusive integer CDF of q, S its total -- what gpf_resample_blocks and gpf_block_moments compute for the block.  Draw j reads resample slot
 * b * n_samples + j of the call's epoch E:
 *     U = resample_u64(seed, b * n_samples + j, E);  target = mulhi64(U, S);  a = the first index with cdf[a] > target, clamped to cnt - 1;
 *     idx_out[b][j] = a + 1.
 * The slots are numbered by draw, not by particle, so the draws of different blocks never share a uniform whatever n_samples is; for ONE block
 * (block_size >= n, n <= 2048) draw j reads slot j, the numbering of gpf_sample_unweighted: the indices equal that call's bit for bit.
 * The path: traj_out[b][j][s - step_lo][c] = trace[s => c] of particle b * block_size + a -- the value gpf_history_column(s, c) holds at that
 * particle -- found by following the composed ancestor maps of the steps T, T-1, ..., s+1.  The ancestor may sit in another block (after
 * gpf_resample_across_blocks or a whole-filter resample).  This is the ancestral path only; gpf_block_backward_sample below is the backward simulation.
 * DEVIATION, as in gpf_block_moments: a block whose log-weights hold a NaN or +Inf gets idx_out = 0 and NaN trajectories; the call succeeds and the
 * other blocks are unaffected (gpf_sample_unweighted on such a sub-state fails).
 * An accepted call advances the RNG epoch once, as gpf_sample_unweighted does, and changes nothing else: rows, weights, parents, log-ML estimate,
 * the "resampled last" mask and the store's records stay.  A refused call changes nothing, the epoch included.  Like the store's other queries
 * the call first materialises anything deferred and snapshots the current step; it synchronises the stream.  The per-block parameter rows are
 * not read (works with gpf_set_block_params).  The device scratch of the results (8 bytes per trajectory cell and per index) is allocated by the
 * call and freed before it returns; the two pointer tables of the walk belong to the store and go with gpf_destroy. */
gpf_status gpf_block_sample_trajectories(gpf_handle h, int64_t block_size, int32_t n_samples, int32_t step_lo, int32_t step_hi,
                                         double* traj_out, int64_t* idx_out);
/* Backward simulation per block (FFBSi: Godsill, Doucet & West 2004; as the path draw of particle Gibbs: Whiteley 2010, Lindsten & Schoen 2013).
 * The ancestral paths of gpf_block_sample_trajectories coalesce: after a few dozen steps all draws of a block share one x_1.  A backward draw
 * re-draws the particle of every earlier step from the step's recorded weights times the model's transition density.
 *
 * gpf_history_enable_blocks_weights is gpf_history_enable_blocks plus two records per step, taken wherever the store takes the latent columns (at the
 * start of the next block-wise step, and at query time for the current one), so both are in the step's FINAL order, after every resample, gather
 * across blocks and rejuvenation of that step:
 *   the n log-weights at that moment -- a block that resampled holds its equal post-resample weights, one the ESS gate left alone its unequal ones;
 *     either is a valid weighted sample of the step's filtering law.  COST: 8 bytes more per particle and step (the store then keeps 8 (dim + 1) n
 *     bytes per step instead of 8 dim n, plus the ancestor map), and one more small launch per snapshot;
 *   the [n_blocks][4] per-block observation rows the step was entered with, in the block order current at the snapshot (gpf_resample_across_blocks
 *     moves them with the blocks).  A step entered by a whole-filter call (gpf_initialize, gpf_update) records no rows and is marked so.
 * Without this mode nothing changes: gpf_history_enable and gpf_history_enable_blocks allocate, launch and compute what they did.
 *
 * gpf_block_backward_sample: ONE launch, all blocks, all draws, all steps.  T = gpf_history_steps, E = the epoch at the call, slot = b n_samples + j.
 *   step T    exactly gpf_block_sample_trajectories' draw from block b's current weights with U = resample_u64(seed, slot, E): the indices at step T
 *             equal that call's on a filter in the same state, bit for bit.
 *   step s    = T-1, ..., step_lo.  p = the particle held in the final order of step s+1, pm = its recorded parent in the final order of step s (the
 *             composed ancestor map of step s+1; p itself where that step had no resample).  The candidates are the particles of block c = pm /
 *             block_size in the snapshot of step s -- the block the held particle was born from: b itself unless gpf_resample_across_blocks moved
 *             it -- with the ancestor weights
 *                 lwa_i = lw_s[i] + logtrans(P_b, x_s[i], x_{s+1}[p], obs_{s+1}[p / block_size])
 *             (Model<M>::logtrans, what gpf_block_ancestor_log_weights adds).  Then as gpf_resample_blocks_ancestor draws its ancestor: maximum and
 *             flags, K = fix_K(particles of block c), q_i = exp_fix(lwa_i - m', K), the inclusive CDF, a = the first index with cdf[a] >
 *             mulhi64(U_s, S') with U_s = resample_u64(seed, slot, E + (T - s)).  The new p = c block_size + a.
 *             P_b is the DRAWING block's CURRENT parameter row under gpf_set_block_params (rows travel with their block, so this is the lineage's
 *             theta), else the filter's: a caller who changes the parameters between steps gets the current ones at every step.
 *   fallback  ancestor weights whose flags hold NaN, +Inf or "all -Inf": the step takes the recorded parent pm (the ancestral step; the ancestor
 *             sampling call falls back to slot 0 likewise).  Otherwise a particle of ancestor weight -Inf is never drawn.
 *   bad block current weights with NaN / +Inf: indices 0 and NaN paths for that block, as gpf_block_sample_trajectories; the others are unaffected.
 *   traj_out  HOST [n_blocks][n_samples][step_hi - step_lo + 1][dim]: the latent columns of the held particle at every step of the range; must not be
 *             NULL.  idx_out: HOST int64, [n_blocks][n_samples][step_hi - step_lo + 1] or NULL: that particle's 1-based GLOBAL index in the final
 *             order of its step.  The walk always starts at T: steps above step_hi are walked, not written.
 *   epoch     an accepted call advances the epoch by T - step_lo + 1 and changes nothing else (rows, weights, parents, log-ML estimate, the "resampled
 *             last" mask, the store's records).  A refused call changes nothing.  Like the other queries it materialises anything deferred,
 *             snapshots the current step and synchronises the stream; the scratch of the results is allocated and freed by the call.
 *   refused   GPF_ERR_STATE: no store, a store without the weight records, a walked step (step_lo < s <= T) entered by a whole-filter call, a clamped
 *             block_size > 2048.  GPF_ERR_INVALID_ARGUMENT: n_samples < 1, n_blocks * n_samples >= 2^31 (or times n_steps * dim), a bad step range,
 *             traj_out NULL, block_size < 1, a block size other than the per-block parameters' or than the one a walked step was entered with.
 * A whole-filter gpf_resample on such a store is walked by the same rule -- the candidates are the recorded parent's block -- but the result is
 * only a valid smoother when every resample was block-wise or across blocks (a whole-filter resample mixes the blocks' weighted samples). */
gpf_status gpf_history_enable_blocks_weights(gpf_handle h, int32_t max_steps);   /* before gpf_initialize_blocks */
gpf_status gpf_block_backward_sample(gpf_handle h, int64_t block_size, int32_t n_samples, int32_t step_lo, int32_t step_hi,
                                     double* traj_out, int64_t* idx_out);
/* Marginal smoothing per block (FFBSm: Hürzeler & Künsch 1998; Doucet, Godsill & Andrieu 2000): deterministic smoothing weights for every particle
 * of every recorded step, and the smoothed mean and variance of every latent column under them,
 *     W_T^j = w_T^j,        W_s^i = sum_j  W_{s+1}^j  w_s^i f(x_{s+1}^j | x_s^i) / sum_l w_s^l f(x_{s+1}^j | x_s^l).
 * A backward draw (gpf_block_backward_sample) gives paths; a smoothed mean from k of them carries Monte-Carlo noise of order 1 / sqrt(k) on top of the
 * particle error.  This call has none: nothing is drawn.  O(block_size^2) transition densities per block and step; ONE launch.
 * Needs gpf_history_enable_blocks_weights.  T = gpf_history_steps, steps s are 1-based, bs = block_size (clamped to n), g_s = the composed ancestor
 * map of step s (the identity where the step had no resample), P_b = the FINAL block b's CURRENT parameter row under gpf_set_block_params, else the
 * filter's.  Every block b < n_blocks is handled independently:
 *   lineage   c_T = b; c_s = g_{s+1}[c_{s+1} bs] / bs: the block the lineage occupied at step s -- b itself unless gpf_resample_across_blocks moved it.
 *             If the particles of block c_{s+1} do not all have their recorded parent in one block (a whole-filter gpf_resample inside a block-wise
 *             step), the lineage is undefined: from step s down block b's outputs are NaN (whole rows of weights_out included) and its blocks_out
 *             entries 0.  The other blocks are unaffected.
 *   step T    W_T^j = (double)q_j / (double)S: block b's current normalised weights as gpf_block_moments forms them (K = fix_K(particles of the block),
 *             q = 1 where all log-weights are -Inf).  Current weights with a NaN or +Inf: every output of block b is NaN at every step, blocks_out 0.
 *   step s    = T-1, ..., step_lo.  Targets j: the particles of block c_{s+1} in the snapshot of step s+1.  Candidates i: the particles of block c_s in
 *             the snapshot of step s.  For each target, in the statements of gpf_block_backward_sample:
 *                 lwa_ij = lw_s[i] + logtrans(P_b, x_s[i], x_{s+1}[j], obs_{s+1}[c_{s+1}]);   (m_j, f_j) = maximum and flags of lwa_.j over i;
 *                 K = fix_K(particles of block c_s);   q_ij = exp_fix(lwa_ij - m_j, K);   D_j = sum_i q_ij (an exact 64-bit integer sum);
 *                 r_ij = (double)q_ij / (double)D_j;
 *             fallback, as in backward simulation: f_j != 0 (NaN, +Inf or all -Inf) -> r_ij = 1 for i = g_{s+1}[j] - c_s bs and 0 otherwise: a target
 *             no candidate leads to hands its mass to its recorded parent.  Then
 *                 W_s^i = sum_j W_{s+1}^j r_ij,
 *             accumulated from +0.0 in ASCENDING j with one multiply and one add per term (no fused multiply-add), not renormalised.  A candidate of
 *             recorded weight -Inf gets W = 0 exactly.
 *   moments   mean_s[c] = tree(W_s^i x_s^i[c]), var_s[c] = tree(W_s^i (x_s^i[c] - mean_s[c])^2): the summation tree of gpf_block_moments
 *             over the index within the block, for all dim latent columns.  At s = T these are gpf_block_moments' values bit for bit.
 *   outputs   HOST, n_steps = step_hi - step_lo + 1: mean_out, var_out [n_blocks][n_steps][dim]; weights_out [n_blocks][n_steps][block_size], indexed
 *             by the particle's position inside block c_s, 0 beyond a short block; blocks_out int64 [n_blocks][n_steps], the 1-based c_s.  Any may be
 *             NULL, not all; what is not asked for is not allocated on the device.  The walk always starts at T: steps above step_hi are walked, not
 *             written.
 *   effects   none: no uniform is read, the epoch does not advance, rows, weights, parents, log-ML estimate, the "resampled last" mask and the store's
 *             records stay.  Like the other queries it materialises anything deferred, snapshots the current step and synchronises the stream.
 *   refused   nothing written, nothing changed.  GPF_ERR_STATE: no store, a store without the weight records, a walked step (step_lo < s <= T) entered
 *             by a whole-filter call, a clamped block_size > 2048.  GPF_ERR_INVALID_ARGUMENT: a bad step range, all outputs NULL, block_size < 1, a block
 *             size other than the per-block parameters' or than the one a walked step was entered with, n_blocks * n_steps * dim or (with weights_out)
 *             n_blocks * n_steps * block_size >= 2^31, a NULL handle. */
gpf_status gpf_block_smooth(gpf_handle h, int64_t block_size, int32_t step_lo, int32_t step_hi,
                            double* mean_out, double* var_out, double* weights_out, int64_t* blocks_out);
/* Pairwise smoothing per block: the E-step of particle EM.  The JOINT smoothed law of two consecutive steps, as lag-one cross moments and second
 * moments, in the same launch that walks the marginal smoother -- E[x_s x_{s+1}^T | y_1:T] and E[x_s x_s^T | y_1:T] are what re-estimating a linear
 * model's transition matrix and noise needs, and for object_motion's `moving` flag the cross moment is the expected transition count.  No
 * block_size x block_size array is stored anywhere: the pairwise weight of (i, j) is the term gpf_block_smooth adds to W_s^i.
 * Everything not named here is gpf_block_smooth's, word for word: T, the lineage c_s, the step-T weights, targets and candidates, lwa_ij, (m_j, f_j), K,
 * q_ij, D_j and r_ij, the fallback to the recorded parent, P_b = the FINAL block's CURRENT parameter row, the walk from T with the steps above
 * step_hi walked and not written, its effects (none: the epoch does not advance) and its refusals.  Needs gpf_history_enable_blocks_weights.
 *   step s    the walk from step s+1 to step s, per candidate i of block c_s: the targets j are taken in ASCENDING order; a target with
 *             W_{s+1}^j == 0 is SKIPPED ENTIRELY (0 * x is not +0.0 for every x); for every other target
 *                 t = W_{s+1}^j * r_ij;    W_s^i = W_s^i + t;    A_i[c] = A_i[c] + t * x_{s+1}^j[c]   for every latent column c,
 *             W_s^i and A_i[c] from +0.0, one multiply and one add per term (no fused multiply-add).  W_s^i is gpf_block_smooth's bit for bit.
 *   outputs   HOST, n_steps = step_hi - step_lo + 1, d = the model's latent dimension, tree = the summation tree of gpf_block_moments
 *             over the index within block c_s, terms beyond a short block +0.0:
 *               mean_out   [n_blocks][n_steps][d]           gpf_block_smooth's mean_out bit for bit;
 *               second_out [n_blocks][n_steps][d][d]        second_s[a][c] = tree_i((W_s^i * x_s^i[a]) * x_s^i[c]) for a <= c; second_s[c][a] is the
 *                                                           same double, mirrored;
 *               cross_out  [n_blocks][n_steps - 1][d][d]    entry o is the pair (s, s+1), s = step_lo + o: cross_s[a][c] = tree_i(x_s^i[a] * A_i[c]),
 *                                                           the particle estimate of E[x_s[a] x_{s+1}[c] | y_1:T];
 *               blocks_out int64 [n_blocks][n_steps]        as in gpf_block_smooth.
 *             Any may be NULL, not all; what is not asked for is not allocated on the device.
 *   undefined a block with NaN / +Inf current weights reads NaN everywhere and lineage 0.  A lineage that is undefined from step s down: NaN for mean
 *             and second of the steps <= s and for every pair whose lower step is <= s.  The other blocks are unaffected.
 *   refused   nothing written, nothing changed.  Those of gpf_block_smooth (GPF_ERR_STATE: no store, a store without the weight records, a walked step
 *             entered by a whole-filter call, a clamped block_size > 2048; GPF_ERR_INVALID_ARGUMENT: a bad step range, block_size < 1, a block size other
 *             than the per-block parameters' or than the one a walked step was entered with, a NULL handle), and GPF_ERR_INVALID_ARGUMENT for all
 *             outputs NULL, cross_out non-NULL with step_lo == step_hi (no pair in the range), n_blocks * n_steps * d * d >= 2^31. */
gpf_status gpf_block_smooth_pairs(gpf_handle h, int64_t block_size, int32_t step_lo, int32_t step_hi,
                                  double* mean_out, double* second_out, double* cross_out, int64_t* blocks_out);

/* The most probable path per block over the grid the block-wise trajectory store holds: the MAP sequence estimator of Godsill, Doucet & West 2001
 * ("Maximum a posteriori sequence estimation using Monte Carlo particle filters", Ann. Inst. Statist. Math. 53) -- particle Viterbi.  For every final
 * block b, over the bs^T sequences that take one particle of the lineage's block at every step 1 .. T (T = gpf_history_steps, bs the clamped block
 * size), the maximiser of
 *     log mu(x_1) + sum_s log f(x_s | x_{s-1}) + sum_s log g(y_s | x_s)
 * by dynamic programming in max-plus form, all blocks and steps in ONE launch, O(T bs^2) logtrans evaluations per block.  The gate, the clamped block
 * size, P_b = the FINAL block's CURRENT parameter row, the step range, materialising deferred work and synchronising the stream are gpf_block_smooth's.
 * Needs gpf_history_enable_blocks_weights: the observation rows are recorded only then (no weight is read).
 *   lineage   c_T = b; c_s = the block ALL recorded parents of the particles of block c_{s+1} sit in (gpf_block_smooth's check).  Where it is undefined
 *             at ANY step, the whole block reads NaN paths, index 0 and logp NaN -- not gpf_block_smooth's rule, on purpose: a recursion that cannot
 *             reach step 1 has no prior term.
 *   node      n_s^i = loglik(P_b, x_s^i, obs_s[c_s]); for s >= 2 and a model with HAS_TRANS_REST: n_s^i = loglik + transrest(P_b, x_s^i, obs_s[c_s])
 *             (one add) -- the part of log f that logtrans drops because it is free of x_{s-1}, but not of x_s (line_model: the outlier's Bernoulli term).
 *   recursion v_T^j = n_T^j.  For s = T-1 .. 1 and every candidate i of block c_s: best = -Inf, ptr = 0; over the targets j of block c_{s+1} in ASCENDING j:
 *                 val = logtrans(P_b, x_s^i, x_{s+1}^j, obs_{s+1}[c_{s+1}]) + v_{s+1}^j;     if (val > best) { best = val; ptr = j; }
 *             so a NaN never wins and the smallest j wins a tie.  v_s^i = n_s^i + best;  ptr_s[i] = ptr.  One add each; no fused multiply-add anywhere.
 *   step 1    tot_i = logprior(P_b, x_1^i, obs_1[c_1]) + v_1^i; i* = the smallest i attaining the maximum of the non-NaN totals, logp[b] = that maximum.
 *             The maximum -Inf (no sequence of positive density on the grid), or every total NaN (then logp = NaN): NaN paths, indices 0.
 *   trace     p_1 = i*, p_{s+1} = ptr_s[p_s].
 *   outputs   HOST, n_steps = step_hi - step_lo + 1, d = the model's latent dimension; the recursion always runs over 1 .. T, the range selects what is written:
 *               path_out [n_blocks][n_steps][d]         path[b][s - step_lo] = the latent columns of particle c_s bs + p_s of snapshot s;
 *               idx_out  int64 [n_blocks][n_steps]      c_s bs + p_s + 1: 1-based, GLOBAL, in the final order of its step (as gpf_block_backward_sample);
 *               logp_out [n_blocks]                     the maximum.
 *             Any may be NULL, not all.
 *   logp      comparable between the paths of ONE block under one parameter row; NOT a normalised log density.  It holds loglik in full, and of log f and
 *             log mu only what depends on the path: the Gaussian normalising constants of the transition and the initial law (T log(sqrt(2 pi) sigma)
 *             terms) and every other term free of x are omitted, as in logtrans.  Because rounded addition is monotone, logp is bit for bit the maximum
 *             over all bs^T sequences of the right-nested total logprior + (n_1 + (lt_12 + (n_2 + (lt_23 + ... + n_T)))).
 *   effects   none: no uniform is read; the epoch does not advance; rows, weights, parents and the store are untouched.  The back-pointers (16-bit, 2 bytes per
 *             particle and step) are device scratch of the call.
 *   refused   nothing written, nothing changed: those of gpf_block_smooth (GPF_ERR_STATE: no store, a store without the weight records, a step entered by a
 *             whole-filter call, a clamped block_size > 2048; GPF_ERR_INVALID_ARGUMENT: a bad step range, block_size < 1, a block size other than the
 *             per-block parameters' or than the one a step was entered with, a NULL handle, all outputs NULL, n_blocks * n_steps * d >= 2^31) -- with every
 *             step 1 .. T a walked step, whatever the range.  Custom proposals: the path is the MAP under the MODEL's densities whatever proposed the grid. */
gpf_status gpf_block_map_path(gpf_handle h, int64_t block_size, int32_t step_lo, int32_t step_hi, double* path_out, int64_t* idx_out, double* logp_out);

/* Forward-only smoothing per block: the sums over steps of gpf_block_smooth_pairs' moments -- sum_s E[x_s x_s^T | y_1:t], sum_s E[x_s x_{s+1}^T | y_1:t],
 * what the M-step of particle EM reads -- after EVERY step, without a store (Del Moral, Doucet & Singh 2010, "Forward smoothing using sequential Monte
 * Carlo"; Poyiadjis, Doucet & Singh 2011, Biometrika 98; the online EM of Cappe 2011).  Every particle carries a statistic T^j of F = d + d(d+1)/2 + d d +
 * d + d(d+1)/2 doubles; one O(bs^2) pass per step updates it from the previous step's particles alone, and sum_j w_t^j T_t^j is algebraically the sum
 * over steps of what gpf_block_smooth_pairs returns.  8 (2 F + d + 1) n bytes and two ancestor maps in all, however long the series.
 * gpf_forward_enable_blocks: before gpf_initialize_blocks*, on an unsharded filter (GPF_ERR_STATE otherwise); with gpf_history_enable_blocks[_weights] on
 * the same handle or with no store at all.  The mode follows the store's "recording" conventions:
 *   step      gpf_initialize_blocks* begins step 1 and resets the statistics; gpf_update_blocks* begins the next step and first CLOSES the step that ends,
 *             in its final order -- after every resample, gather across blocks and rejuvenation of that step, under the per-block observation rows the
 *             step was entered with.  A refused block-wise call closes nothing.
 *   map       g_s, the step's composed ancestor map: gpf_resample_blocks* compose their block-local parents for the blocks that resampled,
 *             gpf_resample_across_blocks its global parents when it fires; several resamples of one step compose in call order.
 *   records   of the previous step only, overwritten at every close: its latent columns, its log-weights, the statistics, the step counter.
 *   size      the clamped block size of the initialising call is the mode's: <= 2048, else GPF_ERR_STATE; a later block-wise step, resample or query with
 *             another clamped block size returns GPF_ERR_INVALID_ARGUMENT.
 *   refused   with the mode on (GPF_ERR_STATE, nothing changed): the whole-filter gpf_initialize*, gpf_update*, gpf_step_ess and gpf_resample* (they
 *             scatter the blocks' lineages), views, gpf_resize / gpf_optimal_resize / gpf_dereplicate / gpf_coalesce / gpf_introduce, gpf_checkpoint_load, a
 *             communicator.  gpf_checkpoint_save saves what it saves without the mode: the statistics are NOT part of a checkpoint.
 * The definition.  Everything not named here is gpf_block_smooth's: logtrans, the maximum and its flags, fix_K, exp_fix, the block's normalised weights.
 * Steps are 1-based, bs = the block size, x = the d latent columns.
 *     T^j = [ sum (d) | second, upper triangle (d(d+1)/2, a <= c, a outer) | cross (d x d, row a = the EARLIER step) | first (d) | first2, upper triangle ]
 *   step 1    sum = first = x_1^j;  second = first2 = x_1^j[a] * x_1^j[c];  cross = +0.0.
 *   step s    >= 2, for every target j of block c = j / bs in the final order of step s:
 *     lineage   pm_j = g_s[j] (j itself where the step had no resample); the candidates are the particles i of block c' = pm_{c bs} / bs in the previous
 *               record.  Where the particles of block c do not all have their parent in one block, every entry of every T of block c is NaN.
 *     weights   lwa_ij = lw_{s-1}[i] + logtrans(P_c, x_{s-1}[i], x_s[j], obs_s[c]); P_c = block c's parameter row CURRENT WHEN THE STEP IS CLOSED
 *               (gpf_set_block_params; rows travel with their block), else the filter's; obs_s[c] = block c's current observation row.
 *               (m_j, f_j) = the maximum and flags over i; K = fix_K(count of c'); q_ij = exp_fix(lwa_ij - m_j, K); D_j = sum_i q_ij (u64, exact).
 *     fallback  f_j != 0 (NaN, +Inf, all -Inf): q_ij = 1 for i = pm_j - c' bs, 0 otherwise, D_j = 1.
 *     sums      over i in ASCENDING order; a candidate with q_ij == 0 is SKIPPED ENTIRELY (0 * x is not +0.0 for every x, and a dead candidate may
 *               carry a non-finite statistic):  h_j[f] = h_j[f] + (double)q_ij * T_{s-1}^i[f];   xb_j[a] = xb_j[a] + (double)q_ij * x_{s-1}^i[a];
 *               both from +0.0, one multiply and one add per term (no fused multiply-add); e_j[f] = h_j[f] / (double)D_j, xbar_j[a] = xb_j[a] / (double)D_j.
 *     new T     sum[a] = e + x_s^j[a];  second[a,c] = e + x_s^j[a] * x_s^j[c];  cross[a][c] = e + xbar_j[a] * x_s^j[c];  first = e;  first2 = e
 *               (e = the entry's own e_j[f]).
 * gpf_block_forward_moments: HOST outputs [n_blocks][d] (sum, first) or [n_blocks][d][d] (second, cross, first2, last2; triangles mirrored); any may be
 * NULL, not all.  It materialises anything deferred, forms the statistics of the CURRENT step as a close would (into scratch: nothing is committed, the
 * close inside the next gpf_update_blocks* recomputes them) and returns
 *     out[b][f] = tree_j(W^j * T^j[f]),      last2_out[b][a][c] = tree_j((W^j * x^j[a]) * x^j[c])   (gpf_block_smooth_pairs' second at the last step)
 * with W^j = (double)q_j / (double)S of the block's current weights and the summation tree of gpf_block_moments over the index within
 * the block.  *n_steps_out = the current step.  The M-step sums follow as second - last2 (steps < t), second - first2 (steps > 1) and cross.
 * A block whose current weights hold NaN / +Inf reads NaN everywhere; the others are unaffected.  No effects: no uniform is read, and epoch, rows, weights,
 * parents and records stay as they are; the stream is synchronised.  Refused: GPF_ERR_STATE -- the mode is off, nothing is initialised;
 * GPF_ERR_INVALID_ARGUMENT -- block_size < 1 or another clamped block size than the mode's, all outputs NULL, a NULL handle. */
gpf_status gpf_forward_enable_blocks(gpf_handle h);   /* before gpf_initialize_blocks */
gpf_status gpf_block_forward_moments(gpf_handle h, int64_t block_size, double* sum_out, double* second_out, double* cross_out, double* first_out,
                                     double* first2_out, double* last2_out, int32_t* n_steps_out);

/* ---- shard-level building blocks (multi-GPU) ------------------------------------------------------
 * A filter sharded over G GPUs is G handles created with the same seed / n_global and contiguous
 * [gid0, gid0 + n_particles) ranges.  gpf_initialize / gpf_update / gpf_rejuvenate work per shard as they
 * are (RNG counters use global particle ids).  Resampling needs one exchange; it is composed from the
 * phases below by the host (sharded.py with torch.distributed = RCCL; a Julia host would use the same
 * calls with MPI.jl/NCCL.jl).  All pointer arguments are DEVICE pointers owned by the caller; every call
 * is asynchronous on the handle's stream.  The reference has no distributed path; these
 * restate src/resample.jl:48-120,143-175 with a global CDF.  Supported here: priority_fn = nothing and
 * sort_particles = false (sort_particles = true: gpf_shard_resample_sorted, the replicated plan).
 *
 *   phase 1  gpf_shard_weight_max     out2 = {local max, local flags & (NaN|+Inf)} as two doubles
 *            host: all-gather -> mf_all[G][2]
 *   phase 2  gpf_shard_weight_scan    in: mf_all (combined in the kernel); local fixed-point CDF; out5 = {S_local, Ql0..3}
 *                                     (the limbs of sum q^2 only when want_q != 0: the ESS needs them, a resample does not)
 *            host: all-gather -> tot_all[G][5]
 *   phase 2b gpf_shard_residual_scan  (residual only) in: tot_all; out2 = {Ctot_local, Rs_local}
 *            host: all-gather -> cr_all[G][2]
 *   phase 3  gpf_shard_push_count     RNG counters are keyed by the GLOBAL slot id, so every shard can work out by itself which
 *                                     output slots draw from ITS part of the global CDF (owner = first shard whose inclusive
 *                                     total exceeds the target): no request message exists.  Multinomial / residual: one pass
 *                                     over the targets of all output slots (residual: the deterministic head in closed form);
 *                                     stratified: the served slots are ONE contiguous range, found in closed form.  The phase
 *                                     also yields the number of entries this shard will send to and receive from each shard
 *                                     (counters cleared by gpf_shard_weight_scan).
 *            host: gpf_shard_counts (the one host sync of a resample: the all-to-all split sizes)
 *   phase 4  gpf_shard_push           ancestor lookup + row gather for every slot this shard owns the target of;
 *                                     packed_out[sum(sent)][W+1] = row | (slot inside its shard) << 32 | global ancestor id,
 *                                     grouped by destination shard (any order inside a group: every entry names its slot).
 *                                     Packs at most `capacity` entries; may be enqueued before gpf_shard_counts (it publishes
 *                                     the counts to pinned host memory when it starts) and called again with a larger buffer
 *                                     if the counts say it overflowed.
 *            host: ONE all-to-all of packed rows (8W+8 bytes per slot that changes shard)
 *   phase 5  gpf_shard_commit         the m = n_particles received entries become the new population: parents, log-weights = 0,
 *                                     log-ML estimate += logsumexp - log N (from mf_all, tot_all).  DEFERRED: the next gpf_update
 *                                     propagates the entries straight out of `packed` into their slots, any other call scatters
 *                                     them first; packed / mf_all / tot_all must stay alive and unchanged until the next
 *                                     gpf_shard_commit on this handle.
 * me = this shard's index; bounds = HOST int64[G+1], first global slot of every shard (bounds[G] = n_global).  G <= 64.
 */
gpf_status gpf_shard_weight_max(gpf_handle h, double* out2);
gpf_status gpf_shard_weight_scan(gpf_handle h, const double* mf_all, int32_t G, int32_t want_q, int64_t* out5);
/* safe_softmax's validity flags of the GLOBAL weights (bit 0 NaN, bit 1 +Inf, bit 2 all -Inf), published to pinned host memory by
 * the last gpf_shard_weight_scan when it starts: the host polls, the stream is not synchronised (check = true / :warn) */
gpf_status gpf_shard_flags(gpf_handle h, int32_t* flags_out);
gpf_status gpf_shard_residual_scan(gpf_handle h, const int64_t* tot_all, int32_t G, int64_t* out2);
gpf_status gpf_shard_push_count(gpf_handle h, int32_t method, const int64_t* tot_all, const int64_t* cr_all, int32_t G, int32_t me,
                                const int64_t* bounds);
/* the counts of the last gpf_shard_push_count as HOST int64[2G] (sent to each shard | received from each shard); synchronises */
gpf_status gpf_shard_counts(gpf_handle h, int32_t G, int64_t* host_counts);
gpf_status gpf_shard_push(gpf_handle h, int32_t method, const int64_t* tot_all, const int64_t* cr_all, int32_t G, int32_t me,
                          const int64_t* bounds, int64_t capacity, double* packed_out);
gpf_status gpf_shard_commit(gpf_handle h, const double* packed, int64_t m, const double* mf_all, const int64_t* tot_all, int32_t G);
/* running log_ml_est of this shard (identical on all shards) */
gpf_status gpf_shard_lml_est(gpf_handle h, double* out);

/* ---- host-side scalar spec (no GPU needed): the same deterministic functions the kernels use ---------- */
int32_t gpf_host_fix_K(int64_t n_global);
/* GPF_RESAMPLE_MULTINOMIAL_SORTED: fixed-point scale of the tile totals; the kernels' reciprocal divisions
 * floor(P 2^64 / den) (P < den < 2^63) and floor(p W / den) (p < den); one tile's gamma variate */
int32_t gpf_host_gamma_E(int64_t n_tiles);
uint64_t gpf_host_div128(uint64_t P, uint64_t den);
uint64_t gpf_host_muldiv128(uint64_t p, uint64_t W, uint64_t den);
uint64_t gpf_host_gamma_tile(uint64_t seed, uint32_t gid, uint32_t epoch, int64_t shape, int32_t Eg);
double  gpf_host_log(double x);
double  gpf_host_lse(double m, uint64_t S, int32_t K, int32_t flags);     /* m + log(S 2^-K) */
double  gpf_host_ess(uint64_t S, uint64_t Q_hi, uint64_t Q_lo);           /* S^2 / Q */
/* ---- the sharded resample behind ONE call (multi-GPU hosts need nothing but these five entry points) -----------------
 * A filter whose handle was created with n_global > n_particles is one shard of a filter spread over `world` processes, one
 * GPU each.  gpf_comm_create gives the handle an RCCL communicator (librccl is loaded with dlopen the first time; nothing is
 * linked against it); gpf_shard_resample then runs the whole global resample of DESIGN.md §6 -- weight maximum, all-gather,
 * fixed-point scan under the global maximum, all-gather of the shard totals (+ the residual counts), push count / push,
 * ONE variable-size exchange of packed rows (grouped ncclSend / ncclRecv: point-to-point pairs over xGMI), deferred commit --
 * on the handle's stream, every collective issued by the library.  It stands in for pf_resample!(state, method; check)
 * (src/resample.jl:19-30) on a sharded state (priority_fn = w -> alpha w: gpf_shard_resample_tempered; sort_particles = true: gpf_shard_resample_sorted).
 *   gpf_comm_unique_id: 128-byte id made by ONE process (ncclGetUniqueId) and handed to all others by the host's own means
 *   (MPI, Distributed.jl, torch.distributed, a file);  rank r of `world` owns the global range [gid0, gid0 + n) its
 *   gpf_config names; ranks are ordered by gid0.
 *   gpf_shard_effective_sample_size / gpf_shard_log_ml_estimate: the getters of src/utils.jl:163-186 over ALL shards
 *   (two all-gathers each; every rank gets the same value). */
gpf_status gpf_comm_unique_id(void* id128);
gpf_status gpf_comm_create(gpf_handle h, const void* id128, int32_t rank, int32_t world);
gpf_status gpf_comm_destroy(gpf_handle h);
/* How the three small summaries of a sharded resample -- (max, flags), {S, sum q^2 limbs}, the residual counts; 16-40 bytes per rank
 *  -- travel: *mailbox = 1: the producing kernel stores them straight into every peer's mailbox (device
 * memory mapped with hipIpc at gpf_comm_create, xGMI peer writes) and the consuming kernel waits for them -- no collective, no
 * launch, no host; 0: RCCL all-gathers (hipIpc mapping not possible on this system, the self-test failed, or GPF_SHARD_SUMMARY=rccl in the environment).
 * Self-test: gpf_comm_create tries the mapped mailboxes out (four dependent rounds between all ranks) and the receive windows below (one entry to and
 * from every peer) before enabling them; one rank whose test fails and every rank keeps RCCL for that transport (GPF_SHARD_SELFTEST=0: no test).
 * Every rank of a communicator is in the same mode.  How the ROWS travel: gpf_comm_set_exchange below. */
gpf_status gpf_comm_summary_mode(gpf_handle h, int32_t* mailbox);
/* exchange volume of this handle's gpf_shard_resample calls so far (what a scaling run compares with the worksheet of DESIGN.md 6.7):
 * out4 = {calls, entries sent to OTHER ranks, entries received from other ranks, bytes of one exchanged entry in the latest call};
 * reset = 1 clears the counters after reading */
gpf_status gpf_comm_traffic(gpf_handle h, int64_t* out4, int32_t reset);

/* The exchange plan of the i.i.d. resamplers (multinomial, and residual's i.i.d. tail) across shards; both give the same bits
 * (Random.rand(Categorical(weights), n), src/resample.jl:59,108 -- every slot's uniform is keyed by its GLOBAL slot id):
 *   GPF_SHARD_PLAN_PUSH (default): every shard evaluates the targets of ALL n_global slots, looks up the ones that fall in its own range
 *     and pushes [row | slot | ancestor] to the slot's shard -- one row exchange, no request message, O(n_global) ALU work per shard;
 *   GPF_SHARD_PLAN_PULL: every shard evaluates only its own n slots and sends each target to its owner, the owners answer with the
 *     rows -- O(n) work per shard, two exchanges and one more host wait.
 * Stratified resampling plans its exchange in closed form and ignores the setting.  Every rank of a communicator must use the same
 * plan.  gpf_comm_create takes the initial plan from the environment (GPF_SHARD_PLAN=push|pull). */
typedef enum { GPF_SHARD_PLAN_PUSH = 0, GPF_SHARD_PLAN_PULL = 1 } gpf_shard_plan;
gpf_status gpf_comm_set_plan(gpf_handle h, int32_t plan);
gpf_status gpf_comm_plan(gpf_handle h, int32_t* plan);
/* How the ROWS of the resamplers with ascending targets travel across shards (stratified with sort_particles = false, src/resample.jl:143-175, and the
 * opt-in sorted multinomial): their exchange is boundary slabs -- a few thousand rows per shard boundary --, i.e. pure latency.
 *   GPF_SHARD_EXCHANGE_P2P (the default wherever the shard mailboxes are up): every rank exports a slot-addressed receive window (one entry per local
 *     slot, hipIpc-mapped by its peers); the merge kernel of the shard that SERVES a slot stores [row | ancestor | seal] straight into the window of the
 *     rank that HOLDS it (xGMI peer stores) and that rank's next gpf_update reads it there, in the same launch as its own slots.  No split sizes for the
 *     host to wait for, no ncclGroup, no send / receive buffers, no capacity to overflow; gpf_shard_resample returns when its kernels are enqueued.
 *   GPF_SHARD_EXCHANGE_RCCL: packed entries, one host wait for the split sizes, grouped ncclSend / ncclRecv (what the i.i.d. resamplers -- a
 *     bandwidth-bound exchange of (G-1)/G of all rows -- and tempered resamples always use).
 * The same bits either way.  Every rank of a communicator must use the same mode.  Environment at gpf_comm_create: GPF_SHARD_EXCHANGE=p2p|p2p_all|rccl. */
/* What the transports under a sharded resample cost on THIS machine -- a scaling run prints it beside its step times (nobody can attach a profiler to it):
 *   out4[0] us per grouped ncclSend / ncclRecv exchange of `entries` packed entries ((W + 1) doubles each) with EVERY peer, mean of `reps` (2 untimed first)
 *   out4[1] the per-link rate of that exchange in GB/s: bytes one rank put on ONE link / out4[0]   (the scaling worksheet of DESIGN.md 6.7 assumes 76)
 *   out4[2] us per mailbox round: every rank stores its entry into every peer's mailbox and waits for all of theirs (`reps` dependent rounds in ONE launch,
 *           the launch's floor out4[3] taken off) -- what each of the 2 - 3 summary rounds of a sharded resample costs between real GPUs
 *   out4[3] us of that launch with no rounds in it
 * Collective: every rank calls it with the same arguments, between resamples.  0 where there is nothing to measure (one rank; no mailboxes). */
gpf_status gpf_comm_calibrate(gpf_handle h, int64_t entries, int32_t reps, double* out4);
typedef enum { GPF_SHARD_EXCHANGE_RCCL = 0, GPF_SHARD_EXCHANGE_P2P = 1,
               /* opt-in: the i.i.d. resamplers' rows (:multinomial, :residual under the push plan; src/resample.jl:59,108) through the windows too -- every entry
                * names its slot, so nothing else changes: no host wait, no ncclGroup for them either.  Their exchange is bandwidth-bound ((G-1)/G of all rows
                * as scattered 8 (W + 2)-byte peer stores against RCCL's bulk copies): which one wins is for a multi-GPU run to say (bench.py --gpus N times both). */
               GPF_SHARD_EXCHANGE_P2P_ALL = 2 } gpf_shard_exchange;
gpf_status gpf_comm_set_exchange(gpf_handle h, int32_t mode);
gpf_status gpf_comm_exchange(gpf_handle h, int32_t* mode);
/* Where the time of a sharded step goes (what a multi-GPU run cannot attach a profiler to): with phase timing on, gpf_shard_resample and the gpf_update that
 * commits it record events on the handle's stream at their phase boundaries.  gpf_phase_times (synchronises): us6 = total microseconds of
 *   [0] summaries   weight maximum -> (max, flags) round -> fixed-point scan -> {S} round (-> residual scans + their round), waits for the peers included
 *   [1] plan        push count: the own-slot search and the pass over the other shards' slots (i.i.d. methods) / the closed-form plan (ascending targets)
 *   [2] pack        look-ups + packing of the served slots (i.i.d.) / merge + own ancestors + window stores or packing (ascending targets)
 *   [3] host wait   WALL CLOCK the host spent blocked on the exchange's split sizes (overlaps [2] on the GPU; 0 for the window exchange)
 *   [4] exchange    grouped ncclSend / ncclRecv + the self copy (0 for the window exchange: its rows travel inside [2])
 *   [5] commit      from the end of the exchange to the end of the next gpf_update's propagate (the host's way back included)
 * over *resamples calls; [0], [1], [2], [4], [5] on the GPU's timeline, idle gaps included.  enable = 1 clears the record. */
enum { GPF_PHASE_SUMMARIES = 0, GPF_PHASE_PLAN = 1, GPF_PHASE_PACK = 2, GPF_PHASE_HOST_WAIT = 3, GPF_PHASE_EXCHANGE = 4, GPF_PHASE_COMMIT = 5, GPF_PHASE_COUNT = 6 };
gpf_status gpf_phase_timing(gpf_handle h, int32_t enable);
gpf_status gpf_phase_times(gpf_handle h, double* us6, int64_t* resamples);
gpf_status gpf_shard_resample(gpf_handle h, int32_t method, int32_t check, int32_t* invalid);
/* pf_resample!(state, method; priority_fn = w -> priority_alpha * w, check) on a sharded state (src/resample.jl:51-52,57,198-200; the
 * tempering family of test/resample.jl:15): ancestors from the CDF of the priorities over ALL shards, log_ml_est from the raw
 * weights, new log-weights log_ws + (log N - logsumexp(log_ws)), log_ws = lw[a] - lp[a], with the logsumexp over all shards.
 * Three summary rounds instead of one and one more double (log_ws) per exchanged entry; the result is bit-identical to
 * gpf_resample(h, method, priority_alpha, ...) on the unsharded filter.  Not together with sort_particles = true. */
gpf_status gpf_shard_resample_tempered(gpf_handle h, int32_t method, double priority_alpha, int32_t check, int32_t* invalid);
/* pf_resample!(state, :stratified; sort_particles = true, check) -- the reference's DEFAULT form of the stratified resampler (src/resample.jl:143-175: strata over
 * the particles in descending weight order, :145,156-157) -- on a sharded state, called on every rank like gpf_shard_resample; the same ancestors as
 * gpf_resample(h, GPF_RESAMPLE_STRATIFIED, NaN, 1, ...) on the unsharded filter, for any number of shards.  A global sort has no shard-local form: every rank
 * gathers ALL log-weights (one all-gather of 8 bytes per global particle) and runs the unsharded sort + scan + search on them itself (a planner filter of
 * n_global particles on every rank, created at the first call; about 130 bytes of HBM per global particle), then serves the rows its particles are ancestors
 * of as packed entries through the grouped point-to-point exchange.  The cost grows with n_global, not with the shard: across shards
 * gpf_shard_resample(GPF_RESAMPLE_STRATIFIED) -- sort_particles = false -- stays the fast form.  No priority_fn. */
gpf_status gpf_shard_resample_sorted(gpf_handle h, int32_t check, int32_t* invalid);
/* ... and its two phases for a host that brings its own collectives (the python engine of sharded.py; cf. gpf_shard_push_count / gpf_shard_push): after the
 * summary phases (gpf_shard_weight_max, gpf_shard_weight_scan), with lw_all = the log-weights of ALL shards in global order on this device (the host's
 * all-gather): gpf_shard_sorted_count runs the planner and leaves the exchange counts for gpf_shard_counts, gpf_shard_sorted_push packs this shard's
 * entries [row | slot << 32 | ancestor id], grouped by destination, at most `capacity` of them; then the exchange and gpf_shard_commit as ever. */
gpf_status gpf_shard_sorted_count(gpf_handle h, const double* lw_all, int32_t G, int32_t me);
gpf_status gpf_shard_sorted_push(gpf_handle h, int32_t G, int32_t me, int64_t capacity, double* packed_out);
/* gpf_step_ess on a sharded filter -- one iteration of the README loop (README.md:66-77), called on every rank like gpf_shard_resample:
 *     if effective_sample_size(state) < ess_frac * N_global;  pf_resample!(state, method);  pf_rejuvenate!(state, ...; method);  end;  pf_update!(state, ...)
 * with the GLOBAL effective sample size; the same results as the separate calls (gpf_shard_effective_sample_size, gpf_shard_resample,
 * gpf_rejuvenate, gpf_update) on every rank.  With the shard mailboxes up, the summary is ONE reduction launch that exchanges the shard totals
 * itself and leaves the verdict on the device, the propagate runs speculatively behind it.  rejuvenate_method < 0: none. */
gpf_status gpf_shard_step_ess(gpf_handle h, const double* obs, int32_t n_obs, double ess_frac, int32_t method, int32_t check,
                              int32_t rejuvenate_method, int32_t n_iters, int32_t* resampled, int32_t* invalid);
gpf_status gpf_shard_effective_sample_size(gpf_handle h, double* out);
gpf_status gpf_shard_log_ml_estimate(gpf_handle h, double* out);

/* test hook: copy one level of the weight CDF left by the last scan of channel 0 to the host.
 * which: 0 cdf (u64 per padded cell), 1 per-16 prefixes (u64), 2 per-256 prefixes (u64), 3 4-byte keys (u32 per 32 cells),
 * 4 16-bit in-group offsets (u16 per padded cell), 5 coarse offset rows (u16).  *n_bytes: capacity in, bytes written out. */
gpf_status gpf_debug_levels(gpf_handle h, int32_t which, void* out, int64_t* n_bytes);

/* host twin of gpf_debug_math (which = 0..5, 7) */
void    gpf_host_math(int32_t which, const double* a, const double* b, int64_t n, double* out, double* out2);

/* ---- checkpoint / resume ----------------------------------------------------------------------
 * No reference counterpart (a Gen ParticleFilterState is an ordinary Julia object: `serialize` does it there).  The whole state of a filter (or of one
 * shard) as ONE host blob: population, log-weights, parents, log-ML estimate, RNG epoch, the latest observation and strata.  gpf_checkpoint_save first
 * turns everything deferred (lazy move, lazy search, un-gathered resample, un-scattered sharded commit) into state; gpf_checkpoint_load takes a handle
 * created with the SAME gpf_config (model, parameters, particle counts, gid0, seed, keep_prev -- else GPF_ERR_INVALID_ARGUMENT) and continues bit for bit
 * where the saved filter stood.  Not part of a blob: the trajectory store (a filter that records one refuses to load), per-block observations, views, the
 * statistics of forward smoothing per block (gpf_forward_enable_blocks: such a filter saves what it would save without the mode and refuses to load). */
gpf_status gpf_checkpoint_size(gpf_handle h, int64_t* bytes);
gpf_status gpf_checkpoint_save(gpf_handle h, void* out, int64_t bytes);
gpf_status gpf_checkpoint_load(gpf_handle h, const void* in, int64_t bytes);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* GPF_H */
