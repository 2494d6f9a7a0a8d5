// libgpf_blocks.hip -- the block-wise filter: many small filters in one state, one launch per call.  Resampling per block (plain, conditional,
// with ancestor sampling) and across blocks, the per-block statistics and estimates, the block-wise initialise / update / rejuvenate with their staged
// observation and reference rows, per-block parameters; blocks of more than BLK_MAX particles go through sub-state views.  The gate and the four small
// helpers the store's queries (libgpf_store.hip) and the forward smoother (libgpf_forward.hip) share with these calls are defined first.
// Buffers: what these calls keep on the handle (per-block masks, statistics, observation / reference / parameter rows, staging) are Dev<T> / Pinned<T>
// members (gpf_host.hpp Owned) that only grow, through grow().
// The per-particle kernels of the block-wise initialise / propagate / move are instantiated elsewhere (launch_init_blk / launch_step_blk / launch_move_blk,
// libgpf_aux.hip, where the reason is given); the block kernels of these calls (gpf_k_block.hpp, gpf_k_block_anc.hpp) here.
#include "gpf_host.hpp"

using namespace gpf;
using namespace gpfh;

namespace gpfh {

// ---- shared with the other units: declared, with their comments, in gpf_host.hpp
gpf_status block_gate(gpf_handle h, int64_t& block_size, const char* who, unsigned steps)
{
    if (!h) return fail(nullptr, GPF_ERR_INVALID_ARGUMENT, "null handle");
    if ((steps & GATE_VIEW) && h->parent) return fail(h, GPF_ERR_STATE, std::string(who) + " on a sub-state view: call it on the filter");
    if ((steps & GATE_SHARD) && h->cfg.n_global != h->n) return fail(h, GPF_ERR_STATE, std::string(who) + " on a shard of a sharded filter");
    if ((steps & GATE_STORE) && h->hist_on && !h->hist_blocks)
        return fail(h, GPF_ERR_STATE, std::string(who) + " on a filter with a trajectory store" + ((steps & GATE_STORE_VIEWS) ? " (it has no sub-state views)" : ""));
    if ((steps & GATE_SIZE) && block_size < 1) return fail(h, GPF_ERR_INVALID_ARGUMENT, "block_size < 1");
    const int64_t clamped = std::min<int64_t>(block_size, std::max<int64_t>(h->n, 1));
    if ((steps & GATE_CLAMP) || ((steps & GATE_CLAMP_STORE) && h->hist_blocks)) block_size = clamped;
    if ((steps & GATE_MAX) && h->hist_blocks && clamped > BLK_MAX)
        return fail(h, GPF_ERR_STATE, std::string(who) + ": blocks of more than " + std::to_string(BLK_MAX) + " particles on a filter with a trajectory store (they would need sub-state views)");
    if ((steps & GATE_PARAMS) && h->bp_size > 0 && block_size != h->bp_size)
        return fail(h, GPF_ERR_INVALID_ARGUMENT, std::string(who) + ": block_size " + std::to_string(block_size) + " differs from the " +
                    std::to_string(h->bp_size) + " of the per-block parameters (gpf_set_block_params)");
    if ((steps & GATE_FWD) && h->fwd_on && h->fwd_steps > 0 && clamped != h->fwd_bsize)
        return fail(h, GPF_ERR_INVALID_ARGUMENT, std::string(who) + ": block_size " + std::to_string(clamped) + " differs from the " +
                    std::to_string(h->fwd_bsize) + " forward smoothing per block was initialised with (gpf_forward_enable_blocks)");
    return GPF_OK;
}
gpf_status block_out(gpf_filter* h, std::initializer_list<OutCopy> outs)
{
    for (const OutCopy& o : outs)
        if (o.host) HIP_TRY(h, hipMemcpyAsync(o.host, o.dev, o.bytes, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return GPF_OK;
}
AncArgs anc_args(const gpf_filter* h)
{
    AncArgs x{};
    for (int i = 0; i < MAX_PARAMS; ++i) x.P[i] = h->args.P[i];
    x.blk_params = h->bp_size > 0 ? h->blk_params : nullptr;
    x.bp_size = h->bp_size > 0 ? h->bp_size : 1;
    return x;
}
gpf_status block_est_buffer(gpf_filter* h, int64_t need) { return h->blk_est.grow(h, (size_t)need); }
BlockMatch make_block_match(const double* values, int32_t n_values)
{
    BlockMatch mv{};
    for (int k = 0; k < BLK_MATCH_MAX; ++k) mv.v[k] = k < n_values ? values[k] : values[n_values - 1];
    mv.n = n_values;
    return mv;
}

namespace {

// METHOD_COND: the conditional multinomial step (slot 0 of every resampling block keeps itself), PRIO = false only
template <int METHOD, int Wc, bool PRIO>
void launch_block_resample_w(gpf_filter* h, const BlockArgs& a)
{
    team_dispatch(a.nb, a.nblocks, [&](auto TEAM, auto ITEMS, dim3 grid) {
        GPF_LAUNCH((k_block_resample<METHOD, Wc, TEAM, ITEMS, PRIO>), grid, dim3(BLOCK), 0, h->stream, a);
    });
}
template <int METHOD>
void launch_block_resample(gpf_filter* h, const BlockArgs& a, bool prio)
{
    if constexpr (METHOD == METHOD_COND) { (void)prio; DISPATCH_W(h, (launch_block_resample_w<METHOD, WW, false>(h, a))); }
    else bool_dispatch(prio, [&](auto PRIO) { DISPATCH_W(h, (launch_block_resample_w<METHOD, WW, PRIO>(h, a))); });
}

// the ancestor-sampling resample (gpf_k_block_anc.hpp): model x keep_prev x team shape; per-block parameters are a run-time branch of the kernel
template <int M, bool KEEP>
void launch_block_resample_anc(gpf_filter* h, const BlockArgs& a, const AncArgs& x)
{
    constexpr int Wc = row_width(Model<M>::D, KEEP);
    team_dispatch(a.nb, a.nblocks, [&](auto TEAM, auto ITEMS, dim3 grid) {
        GPF_LAUNCH((k_block_resample_anc<M, Wc, TEAM, ITEMS>), grid, dim3(BLOCK), 0, h->stream, a, x);
    });
}
template <int M>
void launch_block_anc_lw(gpf_filter* h, const AncArgs& x, int64_t nb, double* out)
{
    const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(4096, (h->n + BLOCK - 1) / BLOCK));
    GPF_LAUNCH((k_block_anc_lw<M>), dim3(grid), dim3(BLOCK), 0, h->stream, x, h->rows[h->cur], h->W, h->lw, h->n, nb, out);
}

// ------------------------------------------------------------------ block-wise resampling: many small filters in one launch (K11)
gpf_status block_buffers(gpf_filter* h, int64_t nblocks)
{
    gpf_status s;
    if (!h->blk_words && (s = h->blk_words.alloc(h, 2))) return s;
    bool fresh = false;
    s = h->blk_mask.grow(h, (size_t)nblocks, &fresh);
    if (fresh) h->blk_last = 0;                                  // the new mask is uninitialised: no block resample to refer to
    return s ? s : h->blk_stats.grow(h, (size_t)nblocks * 2);
}
// the rows of w <= 4 values -> rows of four, zero-padded (the staged observation and reference rows).  Unrolled: at 10^4 blocks this fill is most of
// the host time of a call that stages them
void pack4(double* dst, const double* src, int64_t n_rows, int w)
{
    static_assert(MAX_OBS == 4 && MAX_DIM == 4, "the four columns of a staged row");
    for (int64_t b = 0; b < n_rows; ++b) {
        double* const d = dst + b * 4; const double* const r = src + b * w;
        d[0] = r[0]; d[1] = w > 1 ? r[1] : 0.0; d[2] = w > 2 ? r[2] : 0.0; d[3] = w > 3 ? r[3] : 0.0;
    }
}
// the observations of a block-wise step or of the step an ancestor is sampled towards: [n_blocks][n_obs] with the model's n_obs
gpf_status block_obs_check(gpf_filter* h, const double* obs, int32_t n_obs)
{
    if (obs && n_obs == model_obs_dim(h->cfg.model)) return GPF_OK;
    return fail(h, GPF_ERR_INVALID_ARGUMENT, "this model takes " + std::to_string(model_obs_dim(h->cfg.model)) + " observation values per step and block");
}
// Blocks of more than BLK_MAX = 2048 particles do not fit the one-workgroup-per-block kernels (gpf_k_block.hpp keeps a block's weights, CDF
// and order in LDS).  Their loop over sub-states (for b in blocks; pf_resample!(state[b], ...); end -- test/resample.jl:130-162 has no
// size limit) runs on the host over view handles of the blocks, with the full-size kernels: the same results as the views give, the
// same single epoch for all blocks, no size cliff.  At these sizes a block fills the chip by itself.
gpf_status big_block_views(gpf_filter* h, int64_t block_size)
{
    const int64_t nblocks = (h->n + block_size - 1) / block_size;
    if (h->blk_views_size == block_size && h->blk_views_gen == h->generation && (int64_t)h->blk_views.size() == nblocks) return GPF_OK;
    for (gpf_filter* v : h->blk_views) gpf_destroy(v);
    h->blk_views.clear();
    for (int64_t b = 0; b < nblocks; ++b) {
        gpf_handle v = nullptr;
        const int64_t start = b * block_size, cnt = std::min(block_size, h->n - start);
        gpf_status s = gpf_view_create(h, start, cnt, &v);
        if (s) return s;
        h->blk_views.push_back(v);
    }
    h->blk_views_size = block_size; h->blk_views_gen = h->generation;
    return GPF_OK;
}
// the loop over the sub-states: f(view of block b, b) for every block; a view's failure is the filter's and ends the loop
template <class F>
gpf_status for_big_blocks(gpf_filter* h, int64_t block_size, F&& f)
{
    gpf_status s = big_block_views(h, block_size);
    for (size_t b = 0; !s && b < h->blk_views.size(); ++b) {
        gpf_filter* v = h->blk_views[b];
        if ((s = f(v, (int64_t)b))) h->err = v->err;
    }
    return s;
}
// ---- ancestor sampling: the inputs of the step being entered.  Checked on the host before anything changes; staged into scratch of their own
struct AncestorIn { const double* obs; int32_t n_obs; const double* ref; int32_t n_ref; };
// the reference rows of a pinned step, checked on the host before anything changes: [n_blocks][n_ref] with n_ref = the model's dimension, all finite
gpf_status block_ref_checks(gpf_filter* h, int64_t block_size, const double* ref, int32_t n_ref, const char* who)
{
    const int dim = model_dim(h->cfg.model);
    if (!ref || n_ref != dim)
        return fail(h, GPF_ERR_INVALID_ARGUMENT, std::string(who) + ": the reference has " + std::to_string(dim) + " values per block (the model's latent columns)");
    const int64_t nblocks = (h->n + block_size - 1) / block_size;
    // (one branch-free pass over the exponent fields -- all ones = NaN or +-Inf --, so that the check of 10^4 blocks costs a few microseconds; the
    //  offender is looked for only when there is one)
    uint64_t bad = 0;
    for (int64_t k = 0; k < nblocks * dim; ++k) { uint64_t u; memcpy(&u, ref + k, sizeof(u)); bad |= (uint64_t)(((u >> 52) & 0x7ffu) == 0x7ffu); }
    if (bad)
        for (int64_t k = 0; k < nblocks * dim; ++k)
            if (!(ref[k] - ref[k] == 0.0)) return fail(h, GPF_ERR_INVALID_ARGUMENT, std::string(who) + ": the reference of block " + std::to_string(k / dim) + " is not finite");
    return GPF_OK;
}
gpf_status ancestor_in_checks(gpf_filter* h, int64_t block_size, const AncestorIn& in, const char* who)
{
    if (gpf_status s = block_obs_check(h, in.obs, in.n_obs)) return s;   // (as gpf_update_blocks refuses them)
    return block_ref_checks(h, block_size, in.ref, in.n_ref, who);
}
// [n_blocks][MAX_OBS] data vectors, then [n_blocks][MAX_DIM] reference rows (zero-padded) -> anc_in on the device, by a kernel on the filter's stream;
// x: the kernels' view of them, with the parameters the call uses
gpf_status stage_ancestor_in(gpf_filter* h, int64_t nblocks, const AncestorIn& in, AncArgs& x)
{
    constexpr int ROW = MAX_OBS + MAX_DIM;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    bool fresh = false;
    gpf_status s = h->anc_in.grow(h, (size_t)nblocks * ROW, &fresh);
    if (fresh) h->anc_ev_pending = false;                        // (the stream drained before the old buffers went: nothing reads them any more)
    if (s || (s = h->h_anc_in.grow(h, (size_t)nblocks * ROW))) return s;
    if (!h->anc_ev) HIP_TRY(h, hipEventCreateWithFlags(&h->anc_ev, hipEventDisableTiming));
    if (h->anc_ev_pending) { HIP_TRY(h, hipEventSynchronize(h->anc_ev)); h->anc_ev_pending = false; }   // (the copy that last read the pinned buffer)
    pack4(h->h_anc_in, in.obs, nblocks, in.n_obs);               // (n_obs, dim >= 1: checked)
    pack4(h->h_anc_in + nblocks * MAX_OBS, in.ref, nblocks, model_dim(h->cfg.model));
    const int64_t n_words = nblocks * ROW;
    GPF_LAUNCH(k_stage_words, dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>(64, (n_words + BLOCK - 1) / BLOCK))), dim3(BLOCK), 0, h->stream,
               (const double*)h->h_anc_in.p, h->anc_in.p, n_words);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipEventRecord(h->anc_ev, h->stream));
    h->anc_ev_pending = true;
    x = anc_args(h);
    x.obs = h->anc_in; x.ref = h->anc_in + nblocks * MAX_OBS;
    return GPF_OK;
}
gpf_status resample_big_blocks(gpf_handle h, int32_t method, int64_t block_size, double priority_alpha, int32_t sort_particles,
                                      double ess_frac, int32_t check, int32_t* invalid, int64_t* n_resampled)
{
    gpf_status s = big_block_views(h, block_size);                // (a failure up to here has changed nothing: no bookkeeping)
    const int64_t nblocks = (int64_t)h->blk_views.size();
    if (s || (s = block_buffers(h, nblocks))) return s;
    const uint32_t E = h->epoch;                                 // every block resamples under the call's ONE epoch (like the batched kernel)
    std::vector<int32_t> words((size_t)nblocks, 0);
    bool any_invalid = false, any_nan = false, any_neginf_err = false;
    int64_t count = 0;
    const bool gate = ess_frac == ess_frac && ess_frac >= 0.0;
    // (every view reads its validity flags, also under check = false: a NaN block must be left as it stands, as the batched kernel leaves
    //  it -- which costs one pinned-memory wait per block; at > 2048 particles per block the kernels of the block dominate)
    // a failure other than invalid weights: the loop stops, the bookkeeping below still runs
    const gpf_status hard = for_big_blocks(h, block_size, [&](gpf_filter* v, int64_t b) -> gpf_status {
        h->epoch = E;
        if (gate) {
            double ess = 0.0;
            if (gpf_status es = gpf_effective_sample_size(v, &ess)) return es;
            if (!(ess < ess_frac * (double)v->n)) return GPF_OK; // (an invalid block: ESS NaN -- it does not resample, nothing is reported)
        }
        int32_t inv = 0;
        v->last_flags = 0;
        const gpf_status rs = gpf_resample(v, method, priority_alpha, sort_particles, check == GPF_CHECK_TRUE ? GPF_CHECK_TRUE : GPF_CHECK_WARN, &inv);
        if (rs == GPF_ERR_INVALID_WEIGHTS) {                     // the block is left as it stands; the others go on
            any_invalid = true;
            const bool nan_block = (v->last_flags & (FLAG_NAN | FLAG_POSINF)) != 0;   // (the view's own flags, not its error text)
            if (nan_block) any_nan = true; else any_neginf_err = true;
            words[(size_t)b] = (nan_block ? FLAG_NAN : FLAG_ALL_NEGINF) << 8;      // (the word layout of the batched kernel: flags << 8 | resampled)
            return GPF_OK;
        }
        if (rs) return rs;
        if (inv) { any_invalid = true; words[(size_t)b] |= FLAG_ALL_NEGINF << 8; }
        words[(size_t)b] |= 1;
        ++count;
        return GPF_OK;
    });
    // (also on the error path: the blocks before the failing one HAVE resampled under epoch E -- a later call must not reuse their streams,
    //  the mask must name them and the cached summaries are stale)
    h->epoch = E + 1;
    HIP_TRY(h, hipMemcpyAsync(h->blk_mask, words.data(), (size_t)nblocks * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));                // (the host vector goes out of scope)
    h->blk_last = nblocks;
    weights_written(h, false);
    if (invalid) *invalid = any_invalid ? 1 : 0;
    if (n_resampled) *n_resampled = count;
    if (hard) return hard;
    if (check != GPF_CHECK_FALSE || invalid || n_resampled) {
        if (any_nan) return fail(h, GPF_ERR_INVALID_WEIGHTS, "Invalid weights (NaN).");
        if (check == GPF_CHECK_TRUE && (any_neginf_err || any_invalid)) return fail(h, GPF_ERR_INVALID_WEIGHTS, "Invalid weights.");   // resample.jl:55
    }
    return GPF_OK;
}
// anc != nullptr (conditional only): ancestor sampling -- slot 0 draws its ancestor by the transition density towards the next reference value
gpf_status resample_blocks_impl(gpf_handle h, int32_t method, int64_t block_size, double priority_alpha, int32_t sort_particles,
                                       double ess_frac, int32_t check, int32_t* invalid, int64_t* n_resampled, bool conditional, const AncestorIn* anc = nullptr)
{
    const char* const who = anc ? "gpf_resample_blocks_ancestor" : conditional ? "gpf_resample_blocks_conditional" : "gpf_resample_blocks";
    // (the conditional step has no form for blocks that resample through views: "one block" asked for as any size >= n is one block of n particles)
    gpf_status s = block_gate(h, block_size, who, GATE_FILTER | GATE_FWD | (conditional ? GATE_CLAMP : GATE_CLAMP_STORE | GATE_MAX) | (anc ? GATE_PARAMS : 0u));
    if (s) return s;
    if (conditional && (method == GPF_RESAMPLE_RESIDUAL || method == GPF_RESAMPLE_STRATIFIED))
        return fail(h, GPF_ERR_INVALID_ARGUMENT, std::string(who) + ": multinomial only -- forcing one slot to keep its particle is not a valid conditional scheme "
                    "for residual or stratified resampling (their slots are not exchangeable)");
    if (method != GPF_RESAMPLE_MULTINOMIAL && method != GPF_RESAMPLE_RESIDUAL && method != GPF_RESAMPLE_STRATIFIED)
        return fail(h, GPF_ERR_UNKNOWN_METHOD, "Resampling method not recognized.");          // resample.jl:28
    if (conditional && block_size > BLK_MAX)
        return fail(h, GPF_ERR_INVALID_ARGUMENT, std::string(who) + ": blocks of more than " + std::to_string(BLK_MAX) + " particles resample through sub-state views, which have no conditional form");
    if (anc && (s = ancestor_in_checks(h, block_size, *anc, who))) return s;
    if (h->W != 2 && h->W != 4 && h->W != 8) return fail(h, GPF_ERR_STATE, "row width");
    if ((s = check_ready(h)) || (s = materialize(h))) return s;
    if (block_size > BLK_MAX) return resample_big_blocks(h, method, block_size, priority_alpha, sort_particles, ess_frac, check, invalid, n_resampled);
    const int64_t nblocks = (h->n + block_size - 1) / block_size;
    if ((s = block_buffers(h, nblocks))) return s;
    AncArgs x{};
    if (anc && (s = stage_ancestor_in(h, nblocks, *anc, x))) return s;   // (scratch only: the filter is as it was if this fails)
    BlockArgs a{};
    a.rows_in = h->rows[h->cur]; a.rows_out = h->rows[1 - h->cur]; a.lw = h->lw; a.anc = h->anc;
    a.n = h->n; a.nb = block_size; a.nblocks = nblocks; a.gid0 = h->cfg.gid0; a.seed = h->cfg.seed; a.epoch = h->epoch;
    a.sorted = method == GPF_RESAMPLE_STRATIFIED && sort_particles ? 1 : 0;
    const bool prio = priority_alpha == priority_alpha;
    a.alpha = prio ? priority_alpha : 1.0;
    a.ess_frac = ess_frac == ess_frac ? ess_frac : -1.0;
    a.check_true = check == GPF_CHECK_TRUE ? 1 : 0;
    a.resampled = h->blk_mask;
    s = timed(h, GPF_K_SEARCH, [&] {
        if (anc)                                  bool_dispatch(h->cfg.keep_prev != 0, [&](auto KEEP) { DISPATCH_MODEL(h, (launch_block_resample_anc<MM, KEEP>(h, a, x))); });
        else if (conditional)                     launch_block_resample<METHOD_COND>(h, a, false);
        else if (method == GPF_RESAMPLE_MULTINOMIAL) launch_block_resample<0>(h, a, prio);
        else if (method == GPF_RESAMPLE_RESIDUAL) launch_block_resample<1>(h, a, prio);
        else                                      launch_block_resample<2>(h, a, prio);
    });
    if (s) return s;
    HIP_TRY(h, hipGetLastError());
    h->cur ^= 1;
    h->blk_last = nblocks;
    h->pending_gather = false; h->pending_fill = false;
    h->epoch += 1;
    weights_written(h, false);
    // (the block-wise store: this call's parents into the step's ancestor map -- behind the bookkeeping, so that a failure here leaves a consistent filter)
    if ((s = hist_on_resample(h, block_size))) return s;
    if (check != GPF_CHECK_FALSE || invalid || n_resampled) {
        int32_t words[2] = {0, 0};
        GPF_LAUNCH(k_block_summary, dim3(1), dim3(BLOCK), 0, h->stream, h->blk_mask.p, nblocks, h->blk_words.p);
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipMemcpyAsync(words, h->blk_words, sizeof(words), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        if (invalid) *invalid = words[0] != 0;
        if (n_resampled) *n_resampled = (int64_t)(uint32_t)words[1];
        if (words[0] & (FLAG_NAN | FLAG_POSINF)) return fail(h, GPF_ERR_INVALID_WEIGHTS, "Invalid weights (NaN).");
        if (check == GPF_CHECK_TRUE && words[0]) return fail(h, GPF_ERR_INVALID_WEIGHTS, "Invalid weights.");   // resample.jl:55
    }
    return GPF_OK;
}
// the ESS and the log-ML estimate of every block of <= BLK_MAX particles into blk_stats = [ess | lml] (device)
gpf_status launch_block_stats(gpf_filter* h, int64_t block_size, int64_t nblocks)
{
    gpf_status s = block_buffers(h, nblocks);
    if (s) return s;
    team_dispatch(block_size, nblocks, [&](auto TEAM, auto ITEMS, dim3 grid) {
        GPF_LAUNCH((k_block_stats<TEAM, ITEMS>), grid, dim3(BLOCK), 0, h->stream, h->lw, h->n, block_size, nblocks, &h->sc->lml_est, h->blk_stats.p, h->blk_stats.p + nblocks);
    });
    HIP_TRY(h, hipGetLastError());
    return GPF_OK;
}
template <int Wc>
void launch_block_moments_w(gpf_filter* h, int64_t nb, int64_t nblocks, int want_var, double* mean, double* var)
{
    team_dispatch(nb, nblocks, [&](auto TEAM, auto ITEMS, dim3 grid) {
        GPF_LAUNCH((k_block_moments<Wc, TEAM, ITEMS>), grid, dim3(BLOCK), 0, h->stream, h->rows[h->cur], h->lw, h->n, nb, nblocks, want_var, mean, var);
    });
}
// the gate of the per-block estimates: a filter that can have sub-state views
constexpr unsigned GATE_EST = GATE_FILTER | GATE_STORE_VIEWS | GATE_CLAMP_STORE | GATE_MAX;
// the view of one big block (big_block_views) brought up to date, its weight summary on the host: *bad = NaN / +Inf weights
gpf_status big_block_flags(gpf_filter* v, bool* bad)
{
    gpf_status s = check_ready(v);
    if (s || (s = ensure_raw(v)) || (s = fetch_scalars(v))) return s;
    *bad = (v->h_sc->raw.flags & (FLAG_NAN | FLAG_POSINF)) != 0;
    return GPF_OK;
}
// the blocks' observation vectors -> device ([n_blocks][MAX_OBS], zero-padded), ModelArgs::blk_* set
// ref (a pinned step, [n_blocks][dim], validated by the caller): the reference rows travel behind the observations in the same staging buffer and the
// same launch into blk_ref ([n_blocks][MAX_DIM], zero-padded)
gpf_status set_block_obs(gpf_filter* h, const double* obs, int32_t n_obs, int64_t block_size, const double* ref = nullptr)
{
    gpf_status s = block_obs_check(h, obs, n_obs);
    if (s) return s;
    const int64_t nblocks = (h->n + block_size - 1) / block_size;
    if ((s = h->blk_obs.grow(h, (size_t)nblocks * MAX_OBS))) return s;
    // (MAX_DIM more words per block: the reference rows of a pinned step.  The staging buffers grow with blk_obs and only here;
    //  gpf_resample_across_blocks swaps in a second buffer of at least blk_obs' capacity)
    for (int k = 0; k < gpf_filter::BLK_STAGE; ++k)
        if ((s = h->h_blk_obs[k].grow(h, (size_t)nblocks * (MAX_OBS + MAX_DIM)))) return s;
    if (!h->h_blk_done) {
        if (!h->blk_stage_counter && (s = h->blk_stage_counter.alloc(h, 1))) return s;
        HIP_TRY(h, hipMemsetAsync(h->blk_stage_counter, 0, sizeof(unsigned int), h->stream));
        if ((s = h->h_blk_done.alloc(h, 1))) return s;
        *h->h_blk_done = 0;
    }
    if (ref && (s = h->blk_ref.grow(h, (size_t)nblocks * MAX_DIM))) return s;
    // the staging buffers are used in turn: wait only until the copy that last read THIS buffer (four calls ago) has finished -- its
    // kernel publishes a ticket to pinned memory -- not for the stream
    const int k = (int)(h->blk_stage_next % gpf_filter::BLK_STAGE);
    if (h->blk_stage_next >= gpf_filter::BLK_STAGE) {
        const int64_t need = h->blk_stage_next - gpf_filter::BLK_STAGE + 1;
        const gpf_status ws = poll_published(h, [&] { return __atomic_load_n(h->h_blk_done.p, __ATOMIC_ACQUIRE) >= need; }, nullptr,
                                             "observation staging: the stream drained without the copy's ticket");
        if (ws) return ws;
    }
    h->blk_stage_next += 1;
    double* const stage = h->h_blk_obs[k];
    pack4(stage, obs, nblocks, n_obs);                           // (n_obs = the model's, >= 1: checked above)
    const int64_t n_words = nblocks * MAX_OBS;
    if (ref) {
        pack4(stage + n_words, ref, nblocks, model_dim(h->cfg.model));
        const int64_t n_ref_words = nblocks * MAX_DIM;
        GPF_LAUNCH(k_stage_obs_ref, dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>(64, (n_words + n_ref_words + BLOCK - 1) / BLOCK))), dim3(BLOCK), 0, h->stream,
                   stage, h->blk_obs.p, n_words, h->blk_ref.p, n_ref_words, h->blk_stage_counter.p, h->h_blk_done.p, h->blk_stage_next);
    } else
    GPF_LAUNCH(k_stage_obs, dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>(64, (n_words + BLOCK - 1) / BLOCK))), dim3(BLOCK), 0, h->stream,
               stage, h->blk_obs.p, n_words, h->blk_stage_counter.p, h->h_blk_done.p, h->blk_stage_next);
    HIP_TRY(h, hipGetLastError());
    h->args.blk_obs = h->blk_obs; h->args.blk_mask = nullptr; h->args.blk_size = (int32_t)block_size;
    h->blk_obs_size = block_size;
    return GPF_OK;
}
// the gate of the block-wise steps (they index observations by i / block_size: any size, clamped), then the observations
// initialising: the call sets the block size of forward smoothing per block (at most BLK_MAX, as the store's queries ask); every other step keeps to it
gpf_status block_step_checks(gpf_handle h, int64_t& block_size, const char* who, const double* obs = nullptr, int32_t n_obs = 0, bool with_obs = false,
                                    bool initialising = false)
{
    gpf_status s = block_gate(h, block_size, who, GATE_FILTER | GATE_CLAMP | GATE_PARAMS | (initialising ? 0u : GATE_FWD));
    if (s) return s;
    if (initialising && h->fwd_on && block_size > BLK_MAX)
        return fail(h, GPF_ERR_STATE, std::string(who) + ": blocks of more than " + std::to_string(BLK_MAX) + " particles with forward smoothing per block (gpf_forward_enable_blocks)");
    // (callers that change the handle's arguments before set_block_obs -- the strata -- validate the observations first, so that a bad call changes nothing)
    return with_obs ? block_obs_check(h, obs, n_obs) : GPF_OK;
}
// a block-wise update begins a step of the trajectory store: a full store refuses here, before strata, observations, rows or epoch change
gpf_status block_store_room(gpf_filter* h)
{
    if (h->hist_on && (int)h->hist_x.size() >= h->hist_cap)
        return fail(h, GPF_ERR_STATE, "trajectory store full: raise max_steps of gpf_history_enable");
    return GPF_OK;
}
// The block-wise pf_initialize / pf_update! once the caller's checks (the observations among them: hist_begin_step comes before set_block_obs) have passed (a refused call changes nothing).  mode 0: the default proposal;
// 2: stratified (the caller set the strata); 4 (update): block b is extended with the native proposal where use_proposal[b] != 0.
// ref != nullptr (mode 0 only): slot 0 of every block is pinned to its row of ref (MODE_REF of the kernels).
gpf_status block_initialize_impl(gpf_handle h, const double* obs, int32_t n_obs, int64_t block_size, int mode, const double* ref = nullptr)
{
    h->generation += 1;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    if (h->fwd_on) h->fwd_bsize = block_size;                    // (forward smoothing per block: this call's block size is the mode's)
    gpf_status s = hist_begin_step(h, true);                     // (the block-wise store: step 1)
    if (s || (s = set_block_obs(h, obs, n_obs, block_size, ref))) return s;
    if (h->hist_weights) h->hist_bsize.back() = block_size;     // (the step has per-block observation rows for the store to record)
    if (ref) h->args.blk_ref = h->blk_ref;
    const int grid = step_grid(h);
    s = timed(h, GPF_K_STEP, [&] { launch_init_blk(h, grid, ref ? MODE_REF : mode); });
    h->args.blk_ref = nullptr;                                   // (the reference is this call's input: nothing of it stays)
    if (s || (s = after_initialize(h, grid))) return s;
    h->blk_last = 0;                                             // only_resampled refers to a gpf_resample_blocks of the CURRENT step
    return GPF_OK;
}
gpf_status block_update_impl(gpf_handle h, const double* obs, int32_t n_obs, int64_t block_size, int mode, const int32_t* use_proposal,
                                    const double* ref = nullptr)
{
    gpf_status s = materialize(h);                               // (no fused gather in the block-wise step)
    // (the block-wise store: the step that ends is snapshotted and the next one begins; the entry points have checked the observations and the store's room)
    if (s || (s = hist_begin_step(h, false)) || (s = set_block_obs(h, obs, n_obs, block_size, ref))) return s;
    if (h->hist_weights) h->hist_bsize.back() = block_size;     // (as in block_initialize_impl)
    if (ref) h->args.blk_ref = h->blk_ref;                       // (shares its slot with blk_prop: mode 4 and a reference exclude each other)
    if (mode == 4) {
        const int64_t nblocks = (h->n + block_size - 1) / block_size;
        if ((s = block_buffers(h, nblocks))) return s;           // (blk_mask doubles as the flag array: no block resample refers to it after this call)
        HIP_TRY(h, hipMemcpyAsync(h->blk_mask, use_proposal, (size_t)nblocks * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));             // (the caller's array may go away)
        h->args.blk_prop = h->blk_mask;
    }
    const int grid = step_grid(h);
    s = timed(h, GPF_K_STEP, [&] { launch_step_blk(h, grid, ref ? MODE_REF : mode); });
    h->args.blk_prop = nullptr;
    if (s) return s;
    HIP_TRY(h, hipGetLastError());
    after_propagate(h);
    h->blk_last = 0;                                             // (as in block_initialize_impl)
    return GPF_OK;
}
// for b in blocks: pf_initialize(model, args, observations[b], strata, n_b) / pf_update!(state[b], ..., observations[b], strata) -- stratified
// initialisation / update (src/initialize.jl:92-109, src/update.jl:193-210) of every block by itself, one launch: the stratum of a particle
// follows from its index INSIDE its block and the block's own size (stratified_map!, src/utils.jl:29-55, on the sub-state), the same strata for all blocks
gpf_status block_strata(gpf_handle h, const double* values, int32_t n_strata, int32_t interleaved)
{
    if (!model_caps(h).strata) return fail(h, GPF_ERR_INVALID_ARGUMENT, "this model has no discrete latent to stratify over");
    return set_strata(h, values, n_strata, interleaved);
}
// ------------------------------------------------------------------ resampling ACROSS blocks: the outer level of a nested filter (gpf.h)
// the planner: a filter of n_blocks particles on this filter's stream -- same seed, gid0 = 0 -- that only ever sees log-weights
gpf_status across_planner(gpf_filter* h, int64_t nblocks)
{
    if (h->xb_planner && h->xb_planner->n == nblocks) return GPF_OK;
    if (h->xb_planner) { gpf_destroy(h->xb_planner); h->xb_planner = nullptr; }
    gpf_config c = h->cfg;
    c.n_particles = nblocks; c.n_global = nblocks; c.gid0 = 0; c.keep_prev = 0; c.stream = (void*)h->stream; c.params = h->args.P;
    gpf_handle p = nullptr;
    gpf_status s = gpf_create(&c, &p);
    if (s) return fail(h, s, std::string("planner of gpf_resample_across_blocks: ") + gpf_last_error(nullptr));
    h->xb_planner = p;
    if (p->chain_counted && p->cfg.device < 16) {                // the planner runs on its owner's stream, never beside it (as the planner of the
        std::lock_guard<std::mutex> lk(g_chain[p->cfg.device].mu);   // sorted sharded resample): not one more filter for the gate of chained kernels
        g_chain[p->cfg.device].live -= 1; p->chain_counted = false;
    }
    return GPF_OK;
}

} // namespace
} // namespace gpfh

extern "C" {

gpf_status gpf_resample_blocks(gpf_handle h, int32_t method, int64_t block_size, double priority_alpha, int32_t sort_particles,
                               double ess_frac, int32_t check, int32_t* invalid, int64_t* n_resampled)
{
    return resample_blocks_impl(h, method, block_size, priority_alpha, sort_particles, ess_frac, check, invalid, n_resampled, false);
}
// the conditional multinomial step of conditional SMC (Andrieu, Doucet & Holenstein 2010) for every block -- gpf.h
gpf_status gpf_resample_blocks_conditional(gpf_handle h, int32_t method, int64_t block_size, double ess_frac, int32_t check,
                                           int32_t* invalid, int64_t* n_resampled)
{
    return resample_blocks_impl(h, method, block_size, __builtin_nan(""), 0, ess_frac, check, invalid, n_resampled, true);
}
// particle Gibbs with ancestor sampling (Lindsten, Jordan & Schoen 2014): the conditional step in which slot 0 draws its ancestor -- gpf.h
gpf_status gpf_resample_blocks_ancestor(gpf_handle h, int32_t method, int64_t block_size, double ess_frac, int32_t check,
                                        const double* obs, int32_t n_obs, const double* ref, int32_t n_ref, int32_t* invalid, int64_t* n_resampled)
{
    const AncestorIn in{obs, n_obs, ref, n_ref};
    return resample_blocks_impl(h, method, block_size, __builtin_nan(""), 0, ess_frac, check, invalid, n_resampled, true, &in);
}
gpf_status gpf_block_resampled(gpf_handle h, int32_t* out)
{
    gpf_status s = check_ready(h);
    if (s) return s;
    if (!out) return fail(h, GPF_ERR_INVALID_ARGUMENT, "null out");
    if (!h->blk_mask || h->blk_last < 1) return fail(h, GPF_ERR_STATE, "gpf_block_resampled needs gpf_resample_blocks first");
    HIP_TRY(h, hipMemcpyAsync(out, h->blk_mask, (size_t)h->blk_last * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    for (int64_t i = 0; i < h->blk_last; ++i) out[i] &= 1;       // (the words also carry the blocks' validity flags)
    return GPF_OK;
}
gpf_status gpf_block_stats(gpf_handle h, int64_t block_size, double* ess_out, double* lml_out)
{
    gpf_status s = block_gate(h, block_size, "gpf_block_stats", GATE_VIEW | GATE_SHARD | GATE_SIZE | GATE_CLAMP_STORE | GATE_MAX);
    if (s || (s = check_ready(h)) || (s = materialize(h))) return s;
    const int64_t nblocks = (h->n + block_size - 1) / block_size;
    if (block_size > BLK_MAX)                                    // the loop over sub-states (big_block_views)
        return for_big_blocks(h, block_size, [&](gpf_filter* v, int64_t b) -> gpf_status {
            if (gpf_status es = ess_out ? gpf_effective_sample_size(v, ess_out + b) : GPF_OK) return es;
            return lml_out ? gpf_log_ml_estimate(v, lml_out + b) : GPF_OK;
        });
    if ((s = launch_block_stats(h, block_size, nblocks))) return s;
    const size_t bytes = (size_t)nblocks * sizeof(double);
    return block_out(h, {{h->blk_stats, ess_out, bytes}, {h->blk_stats + nblocks, lml_out, bytes}});
}
// for b in blocks: [mean(state[b], c) for c in columns], [var(state[b], c) ...] (src/statistics.jl:13-14, 48-50 on sub-states) -- gpf.h
gpf_status gpf_block_moments(gpf_handle h, int64_t block_size, double* mean_out, double* var_out)
{
    gpf_status s = block_gate(h, block_size, "gpf_block_moments", GATE_EST);
    if (s) return s;
    if (!mean_out && !var_out) return fail(h, GPF_ERR_INVALID_ARGUMENT, "gpf_block_moments: both outputs are NULL");
    if (h->W != 2 && h->W != 4 && h->W != 8) return fail(h, GPF_ERR_STATE, "row width");
    if ((s = check_ready(h)) || (s = materialize(h))) return s;
    const int64_t nblocks = (h->n + block_size - 1) / block_size;
    const int W = h->W;
    if (block_size > BLK_MAX)                                    // the loop over sub-states (big_block_views)
        return for_big_blocks(h, block_size, [&](gpf_filter* v, int64_t b) -> gpf_status {
            bool bad = false;
            gpf_status vs = big_block_flags(v, &bad);
            for (int c = 0; !vs && c < W; ++c) {
                double* mo = mean_out ? mean_out + b * W + c : nullptr;
                double* vo = var_out ? var_out + b * W + c : nullptr;
                if (bad) { if (mo) *mo = __builtin_nan(""); if (vo) *vo = __builtin_nan(""); continue; }
                if (mo) vs = gpf_mean(v, c, mo);
                if (vo && !vs) vs = gpf_var(v, c, vo);
            }
            return vs;
        });
    const size_t cells = (size_t)nblocks * (size_t)W;
    if ((s = block_est_buffer(h, (int64_t)(2 * cells)))) return s;
    double* const mean = h->blk_est; double* const var = h->blk_est + cells;
    DISPATCH_W(h, (launch_block_moments_w<WW>(h, block_size, nblocks, var_out ? 1 : 0, mean, var)));
    HIP_TRY(h, hipGetLastError());
    return block_out(h, {{mean, mean_out, cells * sizeof(double)}, {var, var_out, cells * sizeof(double)}});
}
// for b in blocks: proportionmap(state[b], column)[values[k]] (src/statistics.jl:91-101 on sub-states) -- gpf.h
gpf_status gpf_block_proportion(gpf_handle h, int64_t block_size, int32_t column, const double* values, int32_t n_values, double* out)
{
    gpf_status s = block_gate(h, block_size, "gpf_block_proportion", GATE_EST);
    if (s) return s;
    if (!values || !out) return fail(h, GPF_ERR_INVALID_ARGUMENT, "gpf_block_proportion: null values / output");
    if (column < 0 || column >= h->W) return fail(h, GPF_ERR_INVALID_ARGUMENT, "bad column");
    if (n_values < 1 || n_values > BLK_MATCH_MAX) return fail(h, GPF_ERR_INVALID_ARGUMENT, "gpf_block_proportion: need 1 <= n_values <= " + std::to_string(BLK_MATCH_MAX));
    if (h->W != 2 && h->W != 4 && h->W != 8) return fail(h, GPF_ERR_STATE, "row width");
    if ((s = check_ready(h)) || (s = materialize(h))) return s;
    const int64_t nblocks = (h->n + block_size - 1) / block_size;
    if (block_size > BLK_MAX)                                    // the loop over sub-states (big_block_views)
        return for_big_blocks(h, block_size, [&](gpf_filter* v, int64_t b) -> gpf_status {
            bool bad = false;
            gpf_status vs = big_block_flags(v, &bad);
            for (int k = 0; !vs && k < n_values; ++k) {
                double* o = out + b * n_values + k;
                if (bad) *o = __builtin_nan(""); else vs = gpf_proportion(v, 0, column, values[k], o);
            }
            return vs;
        });
    const size_t cells = (size_t)nblocks * (size_t)n_values;
    if ((s = block_est_buffer(h, (int64_t)cells))) return s;
    const BlockMatch mv = make_block_match(values, n_values);
    const double* rows = h->rows[h->cur];
    team_dispatch(block_size, nblocks, [&](auto TEAM, auto ITEMS, dim3 grid) {
        GPF_LAUNCH((k_block_proportion<TEAM, ITEMS>), grid, dim3(BLOCK), 0, h->stream, rows, h->W, (int)column, h->lw, h->n, block_size, nblocks, mv, h->blk_est.p);
    });
    HIP_TRY(h, hipGetLastError());
    return block_out(h, {{h->blk_est, out, cells * sizeof(double)}});
}

// lwa_i = lw_i + logtrans(P_b, x_i, ref_b, obs_b) of every particle: the weights the ancestor of slot 0 is drawn from -- gpf.h
gpf_status gpf_block_ancestor_log_weights(gpf_handle h, int64_t block_size, const double* obs, int32_t n_obs, const double* ref, int32_t n_ref, double* out)
{
    const char* const who = "gpf_block_ancestor_log_weights";
    gpf_status s = block_gate(h, block_size, who, GATE_FILTER | GATE_CLAMP);
    if (s) return s;
    const AncestorIn in{obs, n_obs, ref, n_ref};
    if ((s = ancestor_in_checks(h, block_size, in, who))) return s;
    if (!out) return fail(h, GPF_ERR_INVALID_ARGUMENT, std::string(who) + ": null output");
    if ((s = check_ready(h)) || (s = materialize(h))) return s;
    const int64_t nblocks = (h->n + block_size - 1) / block_size;
    AncArgs x{};
    if ((s = block_est_buffer(h, h->n)) || (s = stage_ancestor_in(h, nblocks, in, x))) return s;
    DISPATCH_MODEL(h, (launch_block_anc_lw<MM>(h, x, block_size, h->blk_est)));
    HIP_TRY(h, hipGetLastError());
    return block_out(h, {{h->blk_est, out, (size_t)h->n * sizeof(double)}});
}
gpf_status gpf_initialize_blocks(gpf_handle h, const double* obs, int32_t n_obs, int64_t block_size)
{
    gpf_status s = block_step_checks(h, block_size, "gpf_initialize_blocks", obs, n_obs, true, true);   // (a refused call leaves the trajectory store alone too)
    return s ? s : block_initialize_impl(h, obs, n_obs, block_size, 0);
}
gpf_status gpf_update_blocks(gpf_handle h, const double* obs, int32_t n_obs, int64_t block_size)
{
    gpf_status s = block_step_checks(h, block_size, "gpf_update_blocks", obs, n_obs, true);
    if (s || (s = check_ready(h)) || (s = block_store_room(h))) return s;
    return block_update_impl(h, obs, n_obs, block_size, 0, nullptr);
}
// conditional SMC: the block-wise pf_initialize / pf_update! with slot 0 of every block pinned to a reference row -- gpf.h
gpf_status gpf_initialize_blocks_ref(gpf_handle h, const double* obs, int32_t n_obs, int64_t block_size, const double* ref, int32_t n_ref)
{
    gpf_status s = block_step_checks(h, block_size, "gpf_initialize_blocks_ref", obs, n_obs, true, true);
    if (s || (s = block_ref_checks(h, block_size, ref, n_ref, "gpf_initialize_blocks_ref"))) return s;
    return block_initialize_impl(h, obs, n_obs, block_size, 0, ref);
}
gpf_status gpf_update_blocks_ref(gpf_handle h, const double* obs, int32_t n_obs, int64_t block_size, const double* ref, int32_t n_ref)
{
    gpf_status s = block_step_checks(h, block_size, "gpf_update_blocks_ref", obs, n_obs, true);
    if (s || (s = block_ref_checks(h, block_size, ref, n_ref, "gpf_update_blocks_ref")) || (s = check_ready(h)) || (s = block_store_room(h))) return s;
    return block_update_impl(h, obs, n_obs, block_size, 0, nullptr, ref);
}
gpf_status gpf_initialize_blocks_strata(gpf_handle h, const double* obs, int32_t n_obs, int64_t block_size, const double* values, int32_t n_strata, int32_t interleaved)
{
    gpf_status s = block_step_checks(h, block_size, "gpf_initialize_blocks_strata", obs, n_obs, true, true);
    if (s || (s = block_strata(h, values, n_strata, interleaved))) return s;
    return block_initialize_impl(h, obs, n_obs, block_size, 2);
}
gpf_status gpf_update_blocks_strata(gpf_handle h, const double* obs, int32_t n_obs, int64_t block_size, const double* values, int32_t n_strata, int32_t interleaved)
{
    gpf_status s = block_step_checks(h, block_size, "gpf_update_blocks_strata", obs, n_obs, true);
    if (s || (s = check_ready(h)) || (s = block_store_room(h)) || (s = block_strata(h, values, n_strata, interleaved))) return s;
    return block_update_impl(h, obs, n_obs, block_size, 2, nullptr);
}
// for b in blocks: pf_update!(state[b], new_args, argdiffs, observations[b][, proposal, proposal_args]) -- the per-view updates with DIFFERENT
// proposals per view (test/update.jl:179-189) in one launch: use_proposal[b] != 0 -> block b is extended with the model's native proposal
// (src/update.jl:79-96), else with the default one (src/update.jl:12-25).  One epoch for all blocks, like gpf_update_blocks.
gpf_status gpf_update_blocks_proposal(gpf_handle h, const double* obs, int32_t n_obs, int64_t block_size, const int32_t* use_proposal, int32_t proposal)
{
    gpf_status s = block_step_checks(h, block_size, "gpf_update_blocks_proposal", obs, n_obs, true);
    if (s || (s = check_ready(h)) || (s = block_store_room(h))) return s;
    if (!use_proposal) return fail(h, GPF_ERR_INVALID_ARGUMENT, "null use_proposal");
    if (!proposal_valid(h, proposal) || !model_caps(h).proposal) return fail(h, GPF_ERR_INVALID_ARGUMENT, "this model has no such native proposal");
    return block_update_impl(h, obs, n_obs, block_size, 4, use_proposal);
}
// for t in 1:n_steps; gpf_resample_blocks(check = false); gpf_update_blocks(obs[:, t]); end in one launch (k_block_run, libgpf_run.hip) -- gpf.h.
// Everything up to the input's upload is a check or scratch of the call: a refused call changes nothing
gpf_status gpf_run_blocks(gpf_handle h, const double* obs, int32_t n_obs, int32_t n_steps, int32_t shared_obs, int64_t block_size, int32_t method,
                          int32_t sort_particles, double ess_frac, double* ess_out, double* lml_out, int32_t* resampled_out, int32_t* invalid)
{
    const std::string who = "gpf_run_blocks";
    gpf_status s = block_gate(h, block_size, who.c_str(), GATE_VIEW | GATE_SHARD | GATE_SIZE | GATE_CLAMP | GATE_MAX | GATE_PARAMS | GATE_FWD);
    if (s) return s;
    if (h->hist_on) return fail(h, GPF_ERR_STATE, who + " on a filter with a trajectory store: recording a step is host bookkeeping per step (run the loop of gpf_resample_blocks / gpf_update_blocks)");
    if (h->fwd_on) return fail(h, GPF_ERR_STATE, who + ": forward smoothing per block is on (gpf_forward_enable_blocks): its statistics are closed by a call per step");
    if (h->cfg.keep_prev) return fail(h, GPF_ERR_STATE, who + " on a keep_prev filter: x_{t-1} serves only the rejuvenation moves, and the run has none");
    if (block_size > BLK_MAX) return fail(h, GPF_ERR_INVALID_ARGUMENT, who + ": blocks of more than " + std::to_string(BLK_MAX) + " particles are not the work of one team");
    if (h->args.n_strata > 0) return fail(h, GPF_ERR_STATE, who + ": strata are set on this filter; the run extends every block with the default proposal only");
    if (n_steps < 1 || n_steps > 4096) return fail(h, GPF_ERR_INVALID_ARGUMENT, who + ": need 1 <= n_steps <= 4096 (longer series: call it in chunks, they compose)");
    const int64_t nblocks = (h->n + block_size - 1) / block_size, obs_blocks = shared_obs ? 1 : nblocks;
    if (method != GPF_RESAMPLE_MULTINOMIAL && method != GPF_RESAMPLE_RESIDUAL && method != GPF_RESAMPLE_STRATIFIED)
        return fail(h, GPF_ERR_UNKNOWN_METHOD, "Resampling method not recognized.");          // resample.jl:28
    if ((s = block_obs_check(h, obs, n_obs))) return s;          // (as gpf_update_blocks refuses them: every step's rows have the one width)
    const int64_t obs_words = (int64_t)n_steps * obs_blocks * n_obs;
    if (obs_words > ((int64_t)1 << 31)) return fail(h, GPF_ERR_INVALID_ARGUMENT, who + ": the observations of the call exceed 2^31 words on the device: fewer steps per call");
    // ---- the call's input [MAX_PARAMS parameters | the observations in the caller's layout] into the pinned buffer: ONE pass over the observations,
    //      which is also their check (the exponent fields, branch-free as in block_ref_checks; the offender is looked for only when there is one).
    //      Scratch: a call refused here or below has changed nothing
    const size_t in_words = (size_t)MAX_PARAMS + (size_t)obs_words, cells = (size_t)n_steps * (size_t)nblocks;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    if ((s = h->h_run_in.grow(h, in_words))) return s;
    {
        double* const dst = h->h_run_in + MAX_PARAMS;
        uint64_t bad = 0;
        for (int64_t k = 0; k < obs_words; ++k) { uint64_t u; memcpy(&u, obs + k, sizeof(u)); bad |= (uint64_t)(((u >> 52) & 0x7ffu) == 0x7ffu); memcpy(dst + k, &u, sizeof(u)); }
        if (bad)
            for (int64_t k = 0; k < obs_words; ++k)
                if (!(obs[k] - obs[k] == 0.0)) {
                    const int64_t row = k / n_obs;
                    return fail(h, GPF_ERR_INVALID_ARGUMENT, who + ": the observation of step " + std::to_string(row % n_steps + 1) +
                                (shared_obs ? std::string() : ", block " + std::to_string(row / n_steps)) + " is not finite");
                }
    }
    if (h->W != 2 && h->W != 4) return fail(h, GPF_ERR_STATE, "row width");
    if ((s = check_ready(h)) || (s = materialize(h))) return s;
    // ---- device scratch: the input, the outputs, the words of the summary
    if ((s = block_buffers(h, nblocks)) || (s = h->run_in.grow(h, in_words)) || (s = h->run_stats.grow(h, 2 * cells)) || (s = h->run_words.grow(h, cells)) ||
        (s = h->blk_obs.grow(h, (size_t)nblocks * MAX_OBS))) return s;
    for (int i = 0; i < MAX_PARAMS; ++i) h->h_run_in[i] = h->args.P[i];
    HIP_TRY(h, hipMemcpyAsync(h->run_in, h->h_run_in, in_words * sizeof(double), hipMemcpyHostToDevice, h->stream));
    RunArgs a{};
    a.rows[0] = h->rows[h->cur]; a.rows[1] = h->rows[1 - h->cur]; a.lw = h->lw; a.anc = h->anc;
    a.n = h->n; a.nb = block_size; a.nblocks = nblocks; a.gid0 = h->cfg.gid0; a.seed = h->cfg.seed; a.epoch = h->epoch; a.n_steps = n_steps;
    a.sorted = method == GPF_RESAMPLE_STRATIFIED && sort_particles ? 1 : 0;
    a.ess_frac = ess_frac == ess_frac ? ess_frac : -1.0;
    a.P = h->run_in; a.blk_params = h->bp_size > 0 ? h->blk_params.p : nullptr;
    a.obs = h->run_in + MAX_PARAMS; a.obs_blocks = obs_blocks; a.n_obs = n_obs;
    a.lml_est = &h->sc->lml_est;
    a.ess_out = h->run_stats; a.lml_out = h->run_stats + cells; a.res_out = h->run_words; a.flags_out = h->blk_mask; a.blk_obs = h->blk_obs;
    const int m_id = method == GPF_RESAMPLE_MULTINOMIAL ? 0 : (method == GPF_RESAMPLE_RESIDUAL ? 1 : 2);
    s = timed(h, GPF_K_STEP, [&] { launch_block_run(h, a, m_id); });
    if (s) return s;
    HIP_TRY(h, hipGetLastError());
    // ---- what the loop's 2 n_steps calls leave: two row-buffer flips per iteration (cur as it was), one epoch each, the last step's observation rows
    h->epoch += 2u * (uint32_t)n_steps;
    h->has_prev = true;
    h->pending_gather = false; h->pending_fill = false;
    h->args.blk_obs = h->blk_obs; h->args.blk_mask = nullptr; h->args.blk_size = (int32_t)block_size;
    h->blk_obs_size = block_size;
    h->blk_last = 0;                                             // (blk_mask holds the flag words of the summary below, not a resample's mask)
    weights_written(h, false);
    GPF_LAUNCH(k_block_summary, dim3(1), dim3(BLOCK), 0, h->stream, h->blk_mask.p, nblocks, h->blk_words.p);
    HIP_TRY(h, hipGetLastError());
    int32_t words[2] = {0, 0};
    const size_t bytes = cells * sizeof(double);
    if ((s = block_out(h, {{h->run_stats, ess_out, bytes}, {h->run_stats + cells, lml_out, bytes}, {h->run_words, resampled_out, cells * sizeof(int32_t)},
                           {h->blk_words, words, sizeof(words)}}))) return s;
    if (invalid) *invalid = words[0] != 0;
    if (words[0] & (FLAG_NAN | FLAG_POSINF)) return fail(h, GPF_ERR_INVALID_WEIGHTS, "Invalid weights (NaN).");
    return GPF_OK;
}
gpf_status gpf_rejuvenate_blocks(gpf_handle h, int32_t method, int32_t n_iters, int32_t only_resampled, uint64_t* n_accepted)
{
    gpf_status s = check_ready(h);
    if (s) return s;
    if (h->blk_obs_size < 1) return fail(h, GPF_ERR_STATE, "gpf_rejuvenate_blocks needs gpf_initialize_blocks / gpf_update_blocks first (per-block observations)");
    if ((s = block_step_checks(h, h->blk_obs_size, "gpf_rejuvenate_blocks"))) return s;
    if (method != GPF_REJUVENATE_MOVE && method != GPF_REJUVENATE_REWEIGHT) return fail(h, GPF_ERR_UNKNOWN_METHOD, "Method not recognized.");   // rejuvenate.jl:25
    if (!h->cfg.keep_prev) return fail(h, GPF_ERR_STATE, "gpf_rejuvenate needs keep_prev = 1 (x_{t-1} must travel with the particle)");
    if (n_iters < 0) return fail(h, GPF_ERR_INVALID_ARGUMENT, "n_iters < 0");
    if (only_resampled) {
        const int64_t nblocks = (h->n + h->blk_obs_size - 1) / h->blk_obs_size;
        if (!h->blk_mask || h->blk_last != nblocks) return fail(h, GPF_ERR_STATE, "only_resampled needs a gpf_resample_blocks with the same block size first");
    }
    if ((s = materialize(h))) return s;
    h->args.blk_mask = only_resampled ? h->blk_mask : nullptr;
    const int grid = move_grid(h);
    s = timed(h, GPF_K_MOVE, [&] { launch_move_blk(h, grid, n_iters, method == GPF_REJUVENATE_REWEIGHT); });
    h->args.blk_mask = nullptr;
    if (s) return s;
    HIP_TRY(h, hipGetLastError());
    h->cur ^= 1;
    h->epoch += 1;
    if (method == GPF_REJUVENATE_REWEIGHT) weights_written(h, true);
    else mutated(h);                                             // (a plain move: the weights and their summaries stand)
    if (n_accepted) {
        // (move-reweight: every particle of a participating block moves; the per-workgroup counts cover both cases)
        if (method == GPF_REJUVENATE_REWEIGHT && !only_resampled) *n_accepted = (uint64_t)h->n * (uint64_t)n_iters;
        else if (method == GPF_REJUVENATE_REWEIGHT) {
            int64_t nres = 0;
            GPF_LAUNCH(k_block_summary, dim3(1), dim3(BLOCK), 0, h->stream, h->blk_mask.p, h->blk_last, h->blk_words.p);
            int32_t words[2] = {0, 0};
            HIP_TRY(h, hipMemcpyAsync(words, h->blk_words, sizeof(words), hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(h, hipStreamSynchronize(h->stream));
            nres = (int64_t)(uint32_t)words[1];
            // (all blocks have block_size particles except possibly the last)
            const int64_t bs = h->blk_obs_size, last = h->n - (h->blk_last - 1) * bs;
            int32_t last_word = 0;
            HIP_TRY(h, hipMemcpy(&last_word, h->blk_mask + (h->blk_last - 1), sizeof(int32_t), hipMemcpyDeviceToHost));
            *n_accepted = (uint64_t)((nres - (last_word & 1)) * bs + (last_word & 1) * last) * (uint64_t)n_iters;
        } else {
            GPF_LAUNCH(k_sum_accepts, dim3(1), dim3(BLOCK), 0, h->stream, h->acc_part.p, grid, reinterpret_cast<unsigned long long*>(&h->sc->n_accept));
            HIP_TRY(h, hipGetLastError());
            if ((s = fetch_scalars(h))) return s;
            *n_accepted = h->h_sc->n_accept;
        }
    }
    return GPF_OK;
}
// for b in blocks: the model arguments of state[b] (src/update.jl:12-25 on a sub-state with new_args_b) -- gpf.h gpf_set_block_params.  The rows go
// to the device once, zero-padded to MAX_PARAMS; the block-wise steps read them through ModelArgs::blk_params for as long as they are set
gpf_status gpf_set_block_params(gpf_handle h, const double* params, int32_t n_params, int64_t block_size)
{
    // (a call that clears the rows takes any block size)
    gpf_status s = block_gate(h, block_size, "gpf_set_block_params", GATE_VIEW | GATE_SHARD | GATE_STORE | (params ? GATE_SIZE | GATE_CLAMP : 0u));
    if (s) return s;
    if (!params) {                                               // clear: the filter's own parameter vector again (the buffer stays for reuse)
        h->bp_size = 0; h->args.blk_params = nullptr;
        return GPF_OK;
    }
    if (n_params < 1 || n_params > MAX_PARAMS) return fail(h, GPF_ERR_INVALID_ARGUMENT, "gpf_set_block_params: need 1 <= n_params <= " + std::to_string(MAX_PARAMS));
    const int64_t nblocks = (h->n + block_size - 1) / block_size;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    std::vector<double> rows((size_t)nblocks * MAX_PARAMS, 0.0);
    for (int64_t b = 0; b < nblocks; ++b)
        for (int i = 0; i < n_params; ++i) rows[(size_t)b * MAX_PARAMS + i] = params[b * n_params + i];
    // (kernels enqueued earlier may still read the old rows: the stream drains before the buffer is replaced or overwritten)
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (h->blk_params.count < rows.size()) { h->bp_size = 0; h->args.blk_params = nullptr; }   // (the rows in force go with their buffer)
    if (gpf_status s = h->blk_params.grow(h, rows.size())) return s;
    HIP_TRY(h, hipMemcpyAsync(h->blk_params, rows.data(), rows.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));                 // (the host rows go out of scope)
    h->args.blk_params = h->blk_params;
    h->bp_size = block_size;
    return GPF_OK;
}
// the per-block parameter rows as they stand (after gpf_resample_across_blocks: permuted by its block ancestors) -- gpf.h
gpf_status gpf_get_block_params(gpf_handle h, double* out, int32_t n_params, int64_t n_blocks)
{
    int64_t none = 1;
    if (gpf_status s = block_gate(h, none, "gpf_get_block_params", GATE_VIEW)) return s;
    if (h->bp_size < 1 || !h->blk_params) return fail(h, GPF_ERR_STATE, "gpf_get_block_params: no per-block parameters are set (gpf_set_block_params)");
    const int64_t nblocks = (h->n + h->bp_size - 1) / h->bp_size;
    if (!out || n_params < 1 || n_params > MAX_PARAMS || n_blocks != nblocks)
        return fail(h, GPF_ERR_INVALID_ARGUMENT, "gpf_get_block_params: need an output of [" + std::to_string(nblocks) + "][1 <= n_params <= " + std::to_string(MAX_PARAMS) + "] doubles");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    std::vector<double> rows((size_t)nblocks * MAX_PARAMS);
    HIP_TRY(h, hipMemcpyAsync(rows.data(), h->blk_params, rows.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    for (int64_t b = 0; b < nblocks; ++b)
        for (int i = 0; i < n_params; ++i) out[b * n_params + i] = rows[(size_t)b * MAX_PARAMS + i];
    return GPF_OK;
}

// ---- resampling across blocks (gpf.h): the steps are numbered as there
gpf_status gpf_resample_across_blocks(gpf_handle h, int32_t method, int64_t block_size, int32_t sort_particles, double ess_frac, int32_t check,
                                      int32_t* invalid, int32_t* resampled, double* ess_out)
{
    // (no clamp: the blocks must be congruent, so a size above n is refused below)
    gpf_status s = block_gate(h, block_size, "gpf_resample_across_blocks", GATE_FILTER | GATE_MAX | GATE_PARAMS | GATE_FWD);
    if (s) return s;
    if (h->n % block_size != 0)
        return fail(h, GPF_ERR_INVALID_ARGUMENT, "gpf_resample_across_blocks: " + std::to_string(h->n) + " particles are no whole number of blocks of " +
                    std::to_string(block_size) + " (blocks are copied whole: they must be congruent)");
    if (h->blk_obs_size > 0 && block_size != h->blk_obs_size)
        return fail(h, GPF_ERR_INVALID_ARGUMENT, "gpf_resample_across_blocks: block_size " + std::to_string(block_size) + " differs from the " +
                    std::to_string(h->blk_obs_size) + " of the per-block observations (gpf_update_blocks)");
    if (method != GPF_RESAMPLE_MULTINOMIAL && method != GPF_RESAMPLE_RESIDUAL && method != GPF_RESAMPLE_STRATIFIED)
        return fail(h, GPF_ERR_UNKNOWN_METHOD, "Resampling method not recognized.");          // resample.jl:28
    if (h->W != 2 && h->W != 4 && h->W != 8) return fail(h, GPF_ERR_STATE, "row width");
    if ((s = check_ready(h)) || (s = materialize(h))) return s;
    const int64_t nblocks = h->n / block_size;
    // 1. L[b] = log_ml_estimate(state[b]): the double gpf_block_stats reports
    std::vector<double> L((size_t)nblocks);
    if (block_size > BLK_MAX) {
        if ((s = gpf_block_stats(h, block_size, nullptr, L.data()))) return s;
    } else {
        if ((s = launch_block_stats(h, block_size, nblocks))) return s;
        HIP_TRY(h, hipMemcpyAsync(L.data(), h->blk_stats + nblocks, (size_t)nblocks * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    }
    if ((s = across_planner(h, nblocks))) return s;
    gpf_filter* p = h->xb_planner;
    if (block_size > BLK_MAX) HIP_TRY(h, hipMemcpyAsync(p->lw, L.data(), (size_t)nblocks * sizeof(double), hipMemcpyHostToDevice, h->stream));
    else HIP_TRY(h, hipMemcpyAsync(p->lw, h->blk_stats + nblocks, (size_t)nblocks * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(h, hipMemsetAsync(&p->sc->lml_est, 0, sizeof(double), h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    // 6. invalid weights: a NaN / +Inf estimate = a block with NaN / +Inf weights (refused whatever `check` says); all -Inf
    bool bad = false, all_neginf = true;
    for (double v : L) { if (v != v || v == __builtin_huge_val()) bad = true; if (v != -__builtin_huge_val()) all_neginf = false; }
    if (invalid) *invalid = (bad || all_neginf) ? 1 : 0;
    if (bad) return fail(h, GPF_ERR_INVALID_WEIGHTS, "Invalid weights (NaN).");
    if (all_neginf && check == GPF_CHECK_TRUE) return fail(h, GPF_ERR_INVALID_WEIGHTS, "Invalid weights.");   // resample.jl:55
    // 2. the planner at the call's epoch: ESS, M = logsumexp(L) - log(n_blocks)
    const uint32_t E = h->epoch;
    p->epoch = E; p->initialized = true;
    p->pending_gather = false; p->pending_fill = false; p->pending_search = false;
    weights_written(p, false);
    double ess = 0.0, M = 0.0;
    if ((s = gpf_effective_sample_size(p, &ess)) || (s = gpf_log_ml_estimate(p, &M))) return fail(h, s, "planner: " + p->err);
    if (ess_out) *ess_out = ess;
    // 3. the gate (NaN ESS of all -Inf estimates: `<` is false, like the reference's)
    const bool gated = ess_frac == ess_frac && ess_frac >= 0.0;
    const bool go = !gated || ess < ess_frac * (double)nblocks;
    if (resampled) *resampled = go ? 1 : 0;
    if (go) {
        s = gpf_resample(p, method, __builtin_nan(""), sort_particles, GPF_CHECK_FALSE, nullptr);   // (validity was decided above)
        if (!s) s = finish_search(p);
        p->pending_gather = false; p->pending_fill = false;      // (its ancestors are all this call wants: the planner has no rows worth gathering)
        if (s) return fail(h, s, "planner: " + p->err);
        const bool with_par = h->bp_size > 0, with_obs = h->blk_obs_size > 0;
        // (the second buffer of a per-block row array, at least as large as the first)
        if (with_par && (s = h->blk_params_alt.grow(h, h->blk_params.count))) return s;
        if (with_obs && (s = h->blk_obs_alt.grow(h, h->blk_obs.count))) return s;
        // 4. whole blocks: rows, log-weights + (M - L[a]), parents, per-block rows -- one launch
        BlockGatherArgs a{};
        a.rows_in = h->rows[h->cur]; a.rows_out = h->rows[1 - h->cur]; a.lw_in = h->lw; a.lw_out = h->lws; a.anc_out = h->anc;
        a.A = p->anc; a.L = p->lw; a.M = M;                      // (the planner's weights are untouched by its resample: its gather stays undone)
        a.par_in = with_par ? h->blk_params : nullptr; a.par_out = with_par ? h->blk_params_alt : nullptr;
        a.obs_in = with_obs ? h->blk_obs : nullptr; a.obs_out = with_obs ? h->blk_obs_alt : nullptr;
        a.n = h->n; a.nb = (int32_t)block_size; a.nblocks = (int32_t)nblocks;
        const int64_t chunks = (h->n * (h->W / 2) + BG_PIECES - 1) / BG_PIECES;
        const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(chunks, MAX_PARTIALS));
        s = timed(h, GPF_K_GATHER, [&] { DISPATCH_W(h, GPF_LAUNCH((k_block_gather<WW>), dim3(grid), dim3(BLOCK), 0, h->stream, a)); });
        if (s) return s;
        HIP_TRY(h, hipGetLastError());
        std::vector<int32_t> A((size_t)nblocks);
        HIP_TRY(h, hipMemcpyAsync(A.data(), p->anc, (size_t)nblocks * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        h->xb_anc.resize((size_t)nblocks);
        for (int64_t b = 0; b < nblocks; ++b) h->xb_anc[(size_t)b] = (int64_t)A[(size_t)b] + 1;
        h->xb_anc_gen = h->generation; h->xb_anc_n = h->n;
        h->cur ^= 1;                                             // update_refs! (utils.jl:10-15)
        std::swap(h->lw, h->lws);
        if (with_par) { std::swap(h->blk_params, h->blk_params_alt); h->args.blk_params = h->blk_params; }
        if (with_obs) { std::swap(h->blk_obs, h->blk_obs_alt); h->args.blk_obs = h->blk_obs; }
        h->blk_last = 0;                                         // only_resampled refers to a gpf_resample_blocks of the CURRENT block layout
        weights_written(h, false);
    }
    // 5. one epoch per accepted call, fired or not (as gpf_resample_blocks)
    h->epoch = E + 1;
    // (the block-wise store: h->anc holds global ancestors after a call that fired, as after gpf_resample; one that did not composes nothing)
    return go ? hist_on_resample(h) : GPF_OK;
}
gpf_status gpf_block_ancestors(gpf_handle h, int64_t* out)
{
    if (!h) return fail(nullptr, GPF_ERR_INVALID_ARGUMENT, "null handle");
    if (!out) return fail(h, GPF_ERR_INVALID_ARGUMENT, "null out");
    if (h->xb_anc.empty() || h->xb_anc_gen != h->generation || h->xb_anc_n != h->n)
        return fail(h, GPF_ERR_STATE, "gpf_block_ancestors needs a gpf_resample_across_blocks that resampled first (and no resize since)");
    std::copy(h->xb_anc.begin(), h->xb_anc.end(), out);
    return GPF_OK;
}

} // extern "C"
