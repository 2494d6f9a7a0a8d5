// libgpf_aux.hip -- what widened around the hot path: block-wise operations on many small filters, weighted statistics,
// sub-state views (src/view.jl), the resize family with coalesce / introduce (src/resize.jl), the trajectory store.
// Buffers: what these calls keep on the handle (per-block masks, statistics, observation / reference / parameter rows, staging, the store's snapshots
// and tables) are Dev<T> / Pinned<T> members (gpf_host.hpp Owned) that only grow, through grow(); the scratch of one call is a local Dev<T>.
#include "gpf_host.hpp"
#include "gpf_k_coalesce.hpp"

using namespace gpf;
using namespace gpfh;

namespace gpfh {

// block-wise initialise / propagate / move (ModelArgs::blk_*): no fused gather (a block resample gathers eagerly).  MODE 0: the default proposal;
// 2: stratified; 4 (propagate): per block the native proposal or the default one (ModelArgs::blk_prop).
// BP: per-block parameters are set (gpf_set_block_params) -- the kernels read block b's row of ModelArgs::blk_params instead of P
// MODE_REF: MODE 0 with slot 0 of every block pinned to its reference row (ModelArgs::blk_ref, conditional SMC)
template <int M, int MODE, bool BP>
void launch_init_blk(gpf_filter* h, int grid)
{
    if constexpr (MODE == 2 && !Model<M>::HAS_STRATA) { (void)h; (void)grid; return; }
    else GPF_LAUNCH((k_init<M, MODE, true, BP>), dim3(grid), dim3(BLOCK), 0, h->stream, h->args, h->cfg.seed, h->epoch,
                    h->cfg.gid0, h->n, h->W, h->rows[h->cur], h->lw, next_slots(h));
}
template <int M, int MODE, bool KEEP, bool BP>
void launch_step_blk(gpf_filter* h, int grid)
{
    constexpr int Wc = row_width(Model<M>::D, KEEP);
    if constexpr ((MODE == 2 && !Model<M>::HAS_STRATA) || (MODE == 4 && !Model<M>::HAS_PROPOSAL)) { (void)h; (void)grid; return; }
    else GPF_LAUNCH((k_step<M, Wc, KEEP, false, MODE, false, true, BP>), dim3(grid), dim3(BLOCK), 0, h->stream, h->args, h->cfg.seed, h->epoch,
                    h->cfg.gid0, h->n, h->anc, h->rows[h->cur], h->rows[1 - h->cur], h->lw, next_slots(h), PackedCommit{});
}
template <int M, bool RW, bool BP>
void launch_move_blk(gpf_filter* h, int grid, int n_iters)
{
    constexpr int Wc = row_width(Model<M>::D, true);
    GPF_LAUNCH((k_move<M, Wc, RW, false, false, true, BP>), dim3(grid), dim3(BLOCK), 0, h->stream, h->args, h->cfg.seed, h->epoch,
                       h->cfg.gid0, h->n, (int)h->has_prev, n_iters, h->anc, h->rows[h->cur], h->rows[1 - h->cur], h->lw,
                       h->acc_part.p, RW ? next_slots(h) : MaxSlots{nullptr, nullptr});
}
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

} // namespace gpfh

extern "C" {

// ------------------------------------------------------------------ block-wise resampling: many small filters in one launch (K11)
static gpf_status block_buffers(gpf_filter* h, int64_t nblocks)
{
    gpf_status s;
    if (!h->blk_words && (s = h->blk_words.alloc(h, 2))) return s;
    bool fresh = false;
    s = h->blk_mask.grow(h, (size_t)nblocks, &fresh);
    if (fresh) h->blk_last = 0;                                  // the new mask is uninitialised: no block resample to refer to
    return s ? s : h->blk_stats.grow(h, (size_t)nblocks * 2);
}
// the results of a call from the device to the host, each where the caller wants it (nullptr: not asked for), then the one synchronisation
struct OutCopy { const void* dev; void* host; size_t bytes; };
static gpf_status block_out(gpf_filter* h, std::initializer_list<OutCopy> outs)
{
    for (const OutCopy& o : outs)
        if (o.host) HIP_TRY(h, hipMemcpyAsync(o.host, o.dev, o.bytes, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return GPF_OK;
}
// the rows of w <= 4 values -> rows of four, zero-padded (the staged observation and reference rows).  Unrolled: at 10^4 blocks this fill is most of
// the host time of a call that stages them
static void pack4(double* dst, const double* src, int64_t n_rows, int w)
{
    static_assert(MAX_OBS == 4 && MAX_DIM == 4, "the four columns of a staged row");
    for (int64_t b = 0; b < n_rows; ++b) {
        double* const d = dst + b * 4; const double* const r = src + b * w;
        d[0] = r[0]; d[1] = w > 1 ? r[1] : 0.0; d[2] = w > 2 ? r[2] : 0.0; d[3] = w > 3 ? r[3] : 0.0;
    }
}
// the observations of a block-wise step or of the step an ancestor is sampled towards: [n_blocks][n_obs] with the model's n_obs
static gpf_status block_obs_check(gpf_filter* h, const double* obs, int32_t n_obs)
{
    if (obs && n_obs == model_obs_dim(h->cfg.model)) return GPF_OK;
    return fail(h, GPF_ERR_INVALID_ARGUMENT, "this model takes " + std::to_string(model_obs_dim(h->cfg.model)) + " observation values per step and block");
}
// the parameters a transition density is evaluated with: the filter's own, and the per-block rows where they are set
static AncArgs anc_args(const gpf_filter* h)
{
    AncArgs x{};
    for (int i = 0; i < MAX_PARAMS; ++i) x.P[i] = h->args.P[i];
    x.blk_params = h->bp_size > 0 ? h->blk_params : nullptr;
    x.bp_size = h->bp_size > 0 ? h->bp_size : 1;
    return x;
}
// The preconditions of a block-wise call, in ONE order for every entry point ("the gate of the block-wise calls"); `steps` names the ones
// the entry point has.  Nothing here touches the handle -- check_ready, which brings a lazy move or a view up to date, comes after the gate and after the
// entry point's own checks -- so a refused call changes nothing.  The null handle is refused always.
enum : unsigned {
    GATE_VIEW = 1, GATE_SHARD = 2,
    GATE_STORE = 4,            // a filter with the plain trajectory store (gpf_history_enable) takes no block-wise call
    GATE_STORE_VIEWS = 8,      //   ... and says why: the estimates of big blocks are the work of sub-state views, which it does not have
    GATE_SIZE = 16,            // block_size < 1
    GATE_CLAMP = 32,           // block_size comes back clamped to the particle count: "one block" may be asked for as any size >= n, 2^32 included (the
                               // step kernels divide by it as a 32-bit number, ModelArgs::blk_size, and n < 2^31)
    GATE_CLAMP_STORE = 64,     //   ... only on a filter with the block-wise store (elsewhere a size >= n stays what it is: above BLK_MAX the work of a view)
    GATE_MAX = 128,            // blocks of more than BLK_MAX particles are the work of view handles (below), which a filter with the block-wise store
                               // (gpf_history_enable_blocks) does not have
    GATE_PARAMS = 256,         // the block size of the per-block parameters, where they are set
    GATE_FWD = 512,            // the block size of forward smoothing per block (gpf_forward_enable_blocks), once its initialising call has set it
    GATE_FILTER = GATE_VIEW | GATE_SHARD | GATE_STORE | GATE_SIZE,
};
static gpf_status block_gate(gpf_handle h, int64_t& block_size, const char* who, unsigned steps)
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
// Blocks of more than BLK_MAX = 2048 particles do not fit the one-workgroup-per-block kernels (gpf_k_block.hpp keeps a block's weights, CDF
// and order in LDS).  Their loop over sub-states (for b in blocks; pf_resample!(state[b], ...); end -- test/resample.jl:130-162 has no
// size limit) runs on the host over view handles of the blocks, with the full-size kernels: the same results as the views give, the
// same single epoch for all blocks, no size cliff.  At these sizes a block fills the chip by itself.
static gpf_status big_block_views(gpf_filter* h, int64_t block_size)
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
} // extern "C"
namespace gpfh {
// the loop over the sub-states: f(view of block b, b) for every block; a view's failure is the filter's and ends the loop
template <class F>
static gpf_status for_big_blocks(gpf_filter* h, int64_t block_size, F&& f)
{
    gpf_status s = big_block_views(h, block_size);
    for (size_t b = 0; !s && b < h->blk_views.size(); ++b) {
        gpf_filter* v = h->blk_views[b];
        if ((s = f(v, (int64_t)b))) h->err = v->err;
    }
    return s;
}
} // namespace gpfh
extern "C" {
// ---- ancestor sampling: the inputs of the step being entered.  Checked on the host before anything changes; staged into scratch of their own
struct AncestorIn { const double* obs; int32_t n_obs; const double* ref; int32_t n_ref; };
static gpf_status block_ref_checks(gpf_filter* h, int64_t block_size, const double* ref, int32_t n_ref, const char* who);
static gpf_status ancestor_in_checks(gpf_filter* h, int64_t block_size, const AncestorIn& in, const char* who)
{
    if (gpf_status s = block_obs_check(h, in.obs, in.n_obs)) return s;   // (as gpf_update_blocks refuses them)
    return block_ref_checks(h, block_size, in.ref, in.n_ref, who);
}
// [n_blocks][MAX_OBS] data vectors, then [n_blocks][MAX_DIM] reference rows (zero-padded) -> anc_in on the device, by a kernel on the filter's stream;
// x: the kernels' view of them, with the parameters the call uses
static gpf_status stage_ancestor_in(gpf_filter* h, int64_t nblocks, const AncestorIn& in, AncArgs& x)
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
static gpf_status resample_big_blocks(gpf_handle h, int32_t method, int64_t block_size, double priority_alpha, int32_t sort_particles,
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
static gpf_status resample_blocks_impl(gpf_handle h, int32_t method, int64_t block_size, double priority_alpha, int32_t sort_particles,
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
// the ESS and the log-ML estimate of every block of <= BLK_MAX particles into blk_stats = [ess | lml] (device)
static gpf_status launch_block_stats(gpf_filter* h, int64_t block_size, int64_t nblocks)
{
    gpf_status s = block_buffers(h, nblocks);
    if (s) return s;
    team_dispatch(block_size, nblocks, [&](auto TEAM, auto ITEMS, dim3 grid) {
        GPF_LAUNCH((k_block_stats<TEAM, ITEMS>), grid, dim3(BLOCK), 0, h->stream, h->lw, h->n, block_size, nblocks, &h->sc->lml_est, h->blk_stats.p, h->blk_stats.p + nblocks);
    });
    HIP_TRY(h, hipGetLastError());
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

} // extern "C"

namespace gpfh {
template <int Wc>
void launch_block_moments_w(gpf_filter* h, int64_t nb, int64_t nblocks, int want_var, double* mean, double* var)
{
    team_dispatch(nb, nblocks, [&](auto TEAM, auto ITEMS, dim3 grid) {
        GPF_LAUNCH((k_block_moments<Wc, TEAM, ITEMS>), grid, dim3(BLOCK), 0, h->stream, h->rows[h->cur], h->lw, h->n, nb, nblocks, want_var, mean, var);
    });
}
// the device buffer of the per-block estimates: at least `need` doubles
static gpf_status block_est_buffer(gpf_filter* h, int64_t need) { return h->blk_est.grow(h, (size_t)need); }
// the gate of the per-block estimates: a filter that can have sub-state views
constexpr unsigned GATE_EST = GATE_FILTER | GATE_STORE_VIEWS | GATE_CLAMP_STORE | GATE_MAX;
// the view of one big block (big_block_views) brought up to date, its weight summary on the host: *bad = NaN / +Inf weights
static gpf_status big_block_flags(gpf_filter* v, bool* bad)
{
    gpf_status s = check_ready(v);
    if (s || (s = ensure_raw(v)) || (s = fetch_scalars(v))) return s;
    *bad = (v->h_sc->raw.flags & (FLAG_NAN | FLAG_POSINF)) != 0;
    return GPF_OK;
}
// the match values of a proportion kernel, padded with the last one (the kernels take them two at a time)
static BlockMatch make_block_match(const double* values, int32_t n_values)
{
    BlockMatch mv{};
    for (int k = 0; k < BLK_MATCH_MAX; ++k) mv.v[k] = k < n_values ? values[k] : values[n_values - 1];
    mv.n = n_values;
    return mv;
}
} // namespace gpfh

extern "C" {

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

// the blocks' observation vectors -> device ([n_blocks][MAX_OBS], zero-padded), ModelArgs::blk_* set
// ref (a pinned step, [n_blocks][dim], validated by the caller): the reference rows travel behind the observations in the same staging buffer and the
// same launch into blk_ref ([n_blocks][MAX_DIM], zero-padded)
static gpf_status set_block_obs(gpf_filter* h, const double* obs, int32_t n_obs, int64_t block_size, const double* ref = nullptr)
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
static gpf_status block_step_checks(gpf_handle h, int64_t& block_size, const char* who, const double* obs = nullptr, int32_t n_obs = 0, bool with_obs = false,
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
static gpf_status block_store_room(gpf_filter* h)
{
    if (h->hist_on && (int)h->hist_x.size() >= h->hist_cap)
        return fail(h, GPF_ERR_STATE, "trajectory store full: raise max_steps of gpf_history_enable");
    return GPF_OK;
}
// The block-wise pf_initialize / pf_update! once the caller's checks (the observations among them: hist_begin_step comes before set_block_obs) have passed (a refused call changes nothing).  mode 0: the default proposal;
// 2: stratified (the caller set the strata); 4 (update): block b is extended with the native proposal where use_proposal[b] != 0.
// ref != nullptr (mode 0 only): slot 0 of every block is pinned to its row of ref (MODE_REF of the kernels).
static gpf_status block_initialize_impl(gpf_handle h, const double* obs, int32_t n_obs, int64_t block_size, int mode, const double* ref = nullptr)
{
    h->generation += 1;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    if (h->fwd_on) h->fwd_bsize = block_size;                    // (forward smoothing per block: this call's block size is the mode's)
    gpf_status s = hist_begin_step(h, true);                     // (the block-wise store: step 1)
    if (s || (s = set_block_obs(h, obs, n_obs, block_size, ref))) return s;
    if (h->hist_weights) h->hist_bsize.back() = block_size;     // (the step has per-block observation rows for the store to record)
    if (ref) h->args.blk_ref = h->blk_ref;
    const int grid = step_grid(h);
    s = timed(h, GPF_K_STEP, [&] {
        bool_dispatch(h->bp_size > 0, [&](auto BP) {
            if (ref)            { DISPATCH_MODEL(h, (launch_init_blk<MM, MODE_REF, BP>(h, grid))); }
            else if (mode == 2) { DISPATCH_MODEL(h, (launch_init_blk<MM, 2, BP>(h, grid))); }
            else                { DISPATCH_MODEL(h, (launch_init_blk<MM, 0, BP>(h, grid))); }
        });
    });
    h->args.blk_ref = nullptr;                                   // (the reference is this call's input: nothing of it stays)
    if (s || (s = after_initialize(h, grid))) return s;
    h->blk_last = 0;                                             // only_resampled refers to a gpf_resample_blocks of the CURRENT step
    return GPF_OK;
}
static gpf_status block_update_impl(gpf_handle h, const double* obs, int32_t n_obs, int64_t block_size, int mode, const int32_t* use_proposal,
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
    s = timed(h, GPF_K_STEP, [&] {
        bool_dispatch(h->cfg.keep_prev != 0, h->bp_size > 0, [&](auto KEEP, auto BP) {
            if (ref)            { DISPATCH_MODEL(h, (launch_step_blk<MM, MODE_REF, KEEP, BP>(h, grid))); }
            else if (mode == 4) { DISPATCH_MODEL(h, (launch_step_blk<MM, 4, KEEP, BP>(h, grid))); }
            else if (mode == 2) { DISPATCH_MODEL(h, (launch_step_blk<MM, 2, KEEP, BP>(h, grid))); }
            else                { DISPATCH_MODEL(h, (launch_step_blk<MM, 0, KEEP, BP>(h, grid))); }
        });
    });
    h->args.blk_prop = nullptr;
    if (s) return s;
    HIP_TRY(h, hipGetLastError());
    after_propagate(h);
    h->blk_last = 0;                                             // (as in block_initialize_impl)
    return GPF_OK;
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
// the reference rows of a pinned step, checked on the host before anything changes: [n_blocks][n_ref] with n_ref = the model's dimension, all finite
static gpf_status block_ref_checks(gpf_filter* h, int64_t block_size, const double* ref, int32_t n_ref, const char* who)
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
// for b in blocks: pf_initialize(model, args, observations[b], strata, n_b) / pf_update!(state[b], ..., observations[b], strata) -- stratified
// initialisation / update (src/initialize.jl:92-109, src/update.jl:193-210) of every block by itself, one launch: the stratum of a particle
// follows from its index INSIDE its block and the block's own size (stratified_map!, src/utils.jl:29-55, on the sub-state), the same strata for all blocks
static gpf_status block_strata(gpf_handle h, const double* values, int32_t n_strata, int32_t interleaved)
{
    if (!model_caps(h).strata) return fail(h, GPF_ERR_INVALID_ARGUMENT, "this model has no discrete latent to stratify over");
    return set_strata(h, values, n_strata, interleaved);
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
    s = timed(h, GPF_K_MOVE, [&] {
        bool_dispatch(method == GPF_REJUVENATE_REWEIGHT, h->bp_size > 0, [&](auto RW, auto BP) {
            DISPATCH_MODEL(h, (launch_move_blk<MM, RW, BP>(h, grid, n_iters)));
        });
    });
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

// ------------------------------------------------------------------ resampling ACROSS blocks: the outer level of a nested filter (gpf.h)
// the planner: a filter of n_blocks particles on this filter's stream -- same seed, gid0 = 0 -- that only ever sees log-weights
static gpf_status across_planner(gpf_filter* h, int64_t nblocks)
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

namespace gpfh {
// sum_i w_i f(values[i * stride + col]) by the binary tree of DESIGN.md §3.5 (one workgroup per 2048 terms, then the same tree over
// the partials) into *out_dev (device)
gpf_status weighted_tree_sum(gpf_filter* h, const double* values, int stride, int col, int pw, const double* center, double match, double* out_dev)
{
    const int64_t nb = (h->n + TREE_CHUNK - 1) / TREE_CHUNK;
    const int64_t need = nb + (nb + TREE_CHUNK - 1) / TREE_CHUNK + 1;
    if (gpf_status s = h->tree_buf.grow(h, (size_t)need)) return s;
    double *in = h->tree_buf, *out = h->tree_buf + nb;
    GPF_LAUNCH(k_wsum_tree, dim3((unsigned)nb), dim3(BLOCK), 0, h->stream, h->lw, &h->sc->raw, h->K, values, stride, col, h->n, pw, center, match, in);
    for (int64_t np = nb; np > 1;) {
        const int64_t g = (np + TREE_CHUNK - 1) / TREE_CHUNK;
        GPF_LAUNCH(k_tree_partials, dim3((unsigned)g), dim3(BLOCK), 0, h->stream, in, np, out);
        np = g; std::swap(in, out);
    }
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpyAsync(out_dev, in, sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    return GPF_OK;
}

} // namespace gpfh

extern "C" {

static gpf_status wstat(gpf_handle h, int32_t column, double* out, bool variance)
{
    gpf_status s = check_ready(h);
    if (s) return s;
    if (!out || column < 0 || column >= h->W) return fail(h, GPF_ERR_INVALID_ARGUMENT, "bad column/output");
    if ((s = ensure_raw(h))) return s;
    if ((s = weighted_tree_sum(h, h->rows[h->cur], h->W, column, 1, nullptr, 0.0, h->dscal))) return s;
    if (variance && (s = weighted_tree_sum(h, h->rows[h->cur], h->W, column, 2, h->dscal, 0.0, h->dscal + 1))) return s;
    double tmp[2];
    if ((s = copy_out(h, h->dscal, tmp, sizeof(tmp)))) return s;
    *out = variance ? tmp[1] : tmp[0];
    return GPF_OK;
}
gpf_status gpf_mean(gpf_handle h, int32_t column, double* out) { return wstat(h, column, out, false); }
gpf_status gpf_var(gpf_handle h, int32_t column, double* out) { return wstat(h, column, out, true); }

// =================================================================================== sub-state views (src/view.jl)
gpf_status gpf_view_create(gpf_handle parent, int64_t start, int64_t count, gpf_handle* out)
{
    return gpf_view_create_strided(parent, start, 1, count, out);
}

static gpf_status view_create_impl(gpf_handle parent, int64_t start, int64_t step, int64_t count, const int64_t* index, gpf_handle* out);
gpf_status gpf_view_create_strided(gpf_handle parent, int64_t start, int64_t step, int64_t count, gpf_handle* out)
{
    if (!parent || !out) return fail(parent, GPF_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    if (step < 1 || step >= ((int64_t)1 << 31)) return fail(parent, GPF_ERR_INVALID_ARGUMENT, "view step must be >= 1");
    return view_create_impl(parent, start, step, count, nullptr, out);
}
// state[idxs] / view(state, idxs) for any vector of DISTINCT indices (src/view.jl:35-48): the strided view's compact-copy mechanism with
// an index array.  index: HOST, 0-based, count entries.
gpf_status gpf_view_create_indexed(gpf_handle parent, const int64_t* index, int64_t count, gpf_handle* out)
{
    if (!parent || !out || !index) return fail(parent, GPF_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    if (count < 1) return fail(parent, GPF_ERR_INVALID_ARGUMENT, "empty index vector");
    std::vector<int64_t> sorted(index, index + count);
    std::sort(sorted.begin(), sorted.end());
    if (sorted.front() < 0 || sorted.back() >= parent->n) return fail(parent, GPF_ERR_INVALID_ARGUMENT, "view index out of bounds");
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end())
        return fail(parent, GPF_ERR_INVALID_ARGUMENT, "view indices must be distinct (a particle written through two slots of a view has no defined value)");
    return view_create_impl(parent, index[0], 0, count, index, out);
}
static gpf_status view_create_impl(gpf_handle parent, int64_t start, int64_t step, int64_t count, const int64_t* index, gpf_handle* out)
{
    if (parent->parent) return fail(parent, GPF_ERR_STATE, "views of views are not supported");
    // the trajectory store keeps ONE ancestor map and one set of columns per time step for the whole filter: a sub-state that
    // resamples or advances only its own particles would leave it describing something else -- refuse instead of going stale
    if (parent->hist_on) return fail(parent, GPF_ERR_STATE, "a filter with a trajectory store has no sub-state views");
    if (gpf_status b = fwd_refused(parent, "a sub-state view")) return b;   // (the same reason: one record per step for the whole filter)
    if (!index && (start < 0 || count < 1 || start + (count - 1) * step >= parent->n)) return fail(parent, GPF_ERR_INVALID_ARGUMENT, "view range out of bounds");
    gpf_filter* v = new gpf_filter();
    v->cfg = parent->cfg;
    v->cfg.n_particles = count; v->cfg.n_global = count;          // a sub-state normalises over its own particles
    v->cfg.gid0 = parent->cfg.gid0 + start;                        // ... but RNG counters keep the global particle id
    v->args = parent->args;
    v->d = parent->d; v->W = parent->W; v->n = count; v->n_cu = parent->n_cu;
    v->stream = parent->stream; v->own_stream = false;
    v->parent = parent; v->view_start = start; v->view_step = step; v->parent_generation = parent->generation;
    v->args.gstride = (int32_t)(step ? step : 1);                  // per-particle RNG counters stay the source's particle ids (index views: ModelArgs::gid_map)
    auto body = [&]() -> gpf_status {
        HIP_TRY(v, hipSetDevice(v->cfg.device));
        // scratch of its own (weight levels, descriptors, partials, scalars); rows / lw / anc alias the parent
        gpf_status s;
        if ((s = alloc_particle_buffers(v, true)) || (s = alloc_fixed_buffers(v))) return s;
        const size_t n = (size_t)count;
        if (index) {                                             // the particles' indices in the parent; their ids relative to the first
            std::vector<int32_t> ix((size_t)count), rel((size_t)count);
            for (int64_t i = 0; i < count; ++i) { ix[i] = (int32_t)index[i]; rel[i] = (int32_t)(index[i] - index[0]); }
            if ((s = v->vidx.alloc(v, n)) || (s = v->vgid.alloc(v, n))) return s;
            HIP_TRY(v, hipMemcpy(v->vidx, ix.data(), n * sizeof(int32_t), hipMemcpyHostToDevice));
            HIP_TRY(v, hipMemcpy(v->vgid, rel.data(), n * sizeof(int32_t), hipMemcpyHostToDevice));
            v->args.gid_map = v->vgid;
        }
        if (step != 1 && ((s = v->vrows[0].alloc(v, n * (size_t)v->W)) || (s = v->vrows[1].alloc(v, n * (size_t)v->W)) ||
                          (s = v->vlw.alloc(v, n)) || (s = v->vanc.alloc(v, n)))) return s;
        v->scan_blocks_per_cu = parent->scan_blocks_per_cu; v->wscan_blocks_per_cu = parent->wscan_blocks_per_cu;
        return GPF_OK;
    };
    gpf_status st = body();
    if (st != GPF_OK) { parent->err = v->err; gpf_destroy(v); return st; }
    parent->views.push_back(v);
    *out = v;
    return GPF_OK;
}

// =================================================================================== resize family (src/resize.jl)
// bump = false (gpf_coalesce): the caller makes the views stale itself, once the call can no longer be refused
static gpf_status resize_ready(gpf_handle h, bool bump = true)
{
    if (h && bp_refused(h, "resizing")) return GPF_ERR_STATE;   // (the rows are laid out by block: a new particle count breaks the layout)
    if (h && fwd_refused(h, "resizing")) return GPF_ERR_STATE;  // (the records are laid out by block too)
    gpf_status s = check_ready(h);
    if (s) return s;
    if (h->cfg.n_global != h->n) return fail(h, GPF_ERR_STATE, "resizing a sharded filter is not supported");
    if (h->hist_on) return fail(h, GPF_ERR_STATE, "resizing a filter with a trajectory store is not supported");
    if (h->parent) return fail(h, GPF_ERR_STATE, "a sub-state view cannot be resized");
    if (bump) h->generation += 1;        // views of this filter become stale
    return materialize(h);
}
// after the particle count changed: unsharded bookkeeping
static void set_count(gpf_filter* h, int64_t n_new)
{
    h->n = n_new; h->cfg.n_particles = n_new; h->cfg.n_global = n_new; h->cfg.gid0 = 0;
    if (h->blk_obs_size != 0) h->blk_obs_size = -1;              // per-block observations do not survive a change of the particle count
    h->blk_last = 0;
    // (forget(), not weights_written(): the resize family has never counted a mutation -- the views of a resized filter are stale by its generation)
    h->summary.forget();
    h->pending_gather = false; h->pending_fill = false; h->pending_packed = false; h->pending_search = false;
}

gpf_status gpf_n_particles(gpf_handle h, int64_t* out)
{
    if (!h || !out) return fail(h, GPF_ERR_INVALID_ARGUMENT, "null argument");
    *out = h->n;
    return GPF_OK;
}

// pf_optimal_resize! (resize.jl:149-200): keep every particle with c w_i >= 1, resample the rest by systematic
// sampling, in exact fixed point.  n_new <= n_old.
static gpf_status resize_optimal(gpf_handle h, int64_t n_new, int32_t check, int32_t* invalid)
{
    const int64_t n_old = h->n;
    if (n_new < 1 || n_new > n_old) return fail(h, GPF_ERR_INVALID_ARGUMENT, "optimal resize: need 1 <= n_particles <= current count");   // resize.jl:185
    gpf_status s;
    // sort(weights) (resize.jl:204), descending; safe_softmax + logsumexp (resize.jl:152,190) over that order
    if ((s = ensure_residual_buffers(h))) return s;
    const PrioView pv = raw_view(h);
    if ((s = ensure_max(h, pv, true))) return s;
    if ((s = sort_desc(h, pv, n_old))) return s;
    WSum* ws = &h->sc->raw;
    h->summary.drop_sums();                                      // (cdf[0] is about to hold the scan over the sorted order)
    ScanRequest rq;
    rq.order = h->order; rq.max_ready = true;
    if ((s = summarize(h, pv, ws, rq))) return s;
    HIP_TRY(h, hipMemsetAsync(&h->sc->opt_d, 0xff, sizeof(long long), h->stream));
    GPF_LAUNCH(k_opt_threshold, dim3(grid_for(h, n_new, 8)), dim3(BLOCK), 0, h->stream, h->cdf[0], ws, n_new, n_old, h->sc.p);
    GPF_LAUNCH(k_opt_params, dim3(1), dim3(1), 0, h->stream, h->cdf[0], ws, n_new, h->sc.p);
    // keep flags -> compaction offsets (channel 1); weights of the others -> their CDF (channel 2)
    InOptimal ik{h->lw, ws, h->sc, h->K, 0}, iw{h->lw, ws, h->sc, h->K, 1};
    if ((s = scan_launch_optimal(h, 1, ik, &h->sc->Ctot))) return s;
    if ((s = scan_launch_optimal(h, 2, iw, &h->sc->Rs))) return s;
    if ((s = fetch_scalars(h))) return s;
    const WSum& w = h->h_sc->raw;
    const int64_t n_keep = (int64_t)h->h_sc->Ctot, n_res = n_new - n_keep;
    bool inv = w.flags != 0;
    if ((w.flags & (FLAG_NAN | FLAG_POSINF)) || (check == GPF_CHECK_TRUE && inv)) {
        if (invalid) *invalid = 1;
        return fail(h, GPF_ERR_INVALID_WEIGHTS, "Invalid weights.");                              // resize.jl:153
    }
    if (n_res > 0 && h->h_sc->Rs == 0) {
        // every particle that is not kept has weight 0 at this resolution: uniform among them (safe_softmax, resize.jl:166-168)
        inv = true;
        if (check == GPF_CHECK_TRUE) { if (invalid) *invalid = 1; return fail(h, GPF_ERR_INVALID_WEIGHTS, "Invalid weights."); }
        InOptimal iu{h->lw, ws, h->sc, h->K, 2};
        if ((s = scan_launch_optimal(h, 2, iu, &h->sc->Rs))) return s;
    }
    if (invalid) *invalid = inv ? 1 : 0;
    const CdfLevels lv = levels(h, 2);
    const uint64_t* keepcdf = h->cdf[1];
    const int64_t ntiles_old = h->ntiles;
    const int K = h->K;
    Bufs old = take_particle_buffers(h);
    set_count(h, n_new);
    if ((s = alloc_particle_buffers(h))) { free_bufs(old); return s; }
    GPF_LAUNCH(k_opt_keep_scatter, dim3(grid_for(h, n_old, 8)), dim3(BLOCK), 0, h->stream, keepcdf, n_old, h->anc);
    if (n_res > 0) {
        SearchArgs sa{};
        sa.w = lv; sa.c = lv; sa.ntiles = ntiles_old; sa.order = nullptr; sa.sc = h->sc; sa.ws = ws; sa.raw = ws;
        sa.n = n_res; sa.n_cells = n_old; sa.n_global = n_res; sa.gid0 = 0; sa.seed = h->cfg.seed; sa.epoch = h->epoch;
        sa.K = K; sa.logN = 0.0; sa.update_lml = 0; sa.anc = h->anc + n_keep;
        const size_t lds = search_lds_bytes(ntiles_old, 1);
        const int gsr = (int)std::max<int64_t>(1, std::min<int64_t>((n_res + 2 * SBLOCK - 1) / (2 * SBLOCK), h->n_cu));
        launch_search_plain(h, 3, gsr, lds, sa);
    }
    // new_traces .= view(traces, parents); log_weights (resize.jl:189-197)
    launch_gather_rows_lw(h, h->anc, old.rows[old.cur], old.lw, h->rows[0], h->lw, n_new);
    const double ratio = log_((double)n_new) - log_((double)n_old);
    GPF_LAUNCH(k_opt_weights, dim3(grid_for(h, n_new, 8)), dim3(BLOCK), 0, h->stream, h->lw, n_new, h->sc.p, ws, K, ratio);
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    free_bufs(old);
    HIP_TRY(h, hipGetLastError());
    h->epoch += 1;
    return GPF_OK;
}

gpf_status gpf_resize(gpf_handle h, int64_t n_new, int32_t method, double priority_alpha, int32_t check, int32_t* invalid)
{
    gpf_status s = resize_ready(h);
    if (s) return s;
    if (method == GPF_RESAMPLE_OPTIMAL) return resize_optimal(h, n_new, check, invalid);          // resize.jl:22-23
    if (method != GPF_RESAMPLE_MULTINOMIAL && method != GPF_RESAMPLE_RESIDUAL)
        return fail(h, GPF_ERR_UNKNOWN_METHOD, "Resampling method not recognized.");             // resize.jl:26
    if (n_new < 1 || n_new >= ((int64_t)1 << 31)) return fail(h, GPF_ERR_INVALID_ARGUMENT, "bad n_particles");
    const int64_t n_old = h->n;
    PrioView pv = raw_view(h);
    if (priority_alpha == priority_alpha) { pv.alpha = priority_alpha; pv.mode = 1; }
    // fixed-point scale for max(n_old, n_new): both N_old 2^K and n_new 2^K must stay below 2^62
    h->K = fix_K(std::max(n_old, n_new));
    h->summary.drop_sums();                                      // (sums at another K)
    WSum* ws = &h->sc->raw;
    ScanRequest rq;
    rq.producer_max = true;
    if ((s = summarize(h, raw_view(h), &h->sc->raw, rq))) return s;                            // logsumexp(log_weights), resize.jl:58
    rq.producer_max = false;
    if (pv.mode != 0) { ws = &h->sc->prio; if ((s = summarize(h, pv, ws, rq))) return s; }
    if (check == GPF_CHECK_TRUE || invalid) {
        if ((s = fetch_scalars(h))) return s;
        const WSum& w = pv.mode == 0 ? h->h_sc->raw : h->h_sc->prio;
        if (invalid) *invalid = w.flags != 0;
        if ((w.flags & (FLAG_NAN | FLAG_POSINF)) || (check == GPF_CHECK_TRUE && w.flags)) {
            h->K = fix_K(n_old);
            return fail(h, GPF_ERR_INVALID_WEIGHTS, "Invalid weights.");                          // resize.jl:56,97
        }
    }
    SearchArgs sa{};
    sa.w = levels(h, 0); sa.c = levels(h, 0); sa.ntiles = h->ntiles; sa.order = nullptr; sa.sc = h->sc; sa.ws = ws;
    sa.raw = &h->sc->raw; sa.n = n_new; sa.n_cells = n_old; sa.n_global = n_new; sa.gid0 = 0; sa.seed = h->cfg.seed;
    sa.epoch = h->epoch; sa.K = h->K; sa.logN = log_((double)n_old); sa.update_lml = 1;
    if (method == GPF_RESAMPLE_RESIDUAL) {
        if ((s = residual_scans(h, ws, n_new))) return s;                                        // floor(n_particles * w), resize.jl:106
        sa.w = levels(h, 2); sa.c = levels(h, 1);
    }
    const int64_t ntiles_old = h->ntiles;
    const int Kp = h->K;
    Bufs old = take_particle_buffers(h);                                                          // resize!(...), resize.jl:60-61
    set_count(h, n_new);
    if ((s = alloc_particle_buffers(h))) { free_bufs(old); return s; }
    sa.anc = h->anc;
    const int64_t nt = method == GPF_RESAMPLE_RESIDUAL ? 2 : 1;
    const size_t lds = search_lds_bytes(ntiles_old, (int)nt);
    const int gsr = (int)std::max<int64_t>(1, std::min<int64_t>((n_new + 2 * SBLOCK - 1) / (2 * SBLOCK), h->n_cu));
    if (method == GPF_RESAMPLE_RESIDUAL) launch_search_plain(h, 1, gsr, lds, sa);
    else                                 launch_multinomial_search(h, sa);
    // new_traces .= view(traces, parents) + update_weights!(state, n_particles, log_priorities)   resize.jl:64-66,424-438
    launch_gather_ex(h, h->anc, old.rows[old.cur], h->rows[0], pv, pv.mode == 0 ? h->lw : h->lws, n_new);
    if (pv.mode != 0) {
        PrioView post{h->lws, nullptr, 0.0, 0};
        rq.cdf = false;
        if ((s = summarize(h, post, &h->sc->post, rq))) { free_bufs(old); return s; }
        GPF_LAUNCH(k_apply_post, dim3(grid_for(h, n_new, 8)), dim3(BLOCK), 0, h->stream, h->sc.p, h->K, h->logN, h->lws, h->lw, n_new);      // (the slots describe log_ws: ensure_max said so)
    }
    (void)Kp;
    HIP_TRY(h, hipStreamSynchronize(h->stream));                 // the old buffers are read by the kernels above
    free_bufs(old);
    HIP_TRY(h, hipGetLastError());
    h->epoch += 1;
    return GPF_OK;
}

gpf_status gpf_replicate(gpf_handle h, int32_t n_replicates, int32_t interleaved)
{
    gpf_status s = resize_ready(h);
    if (s) return s;
    if (n_replicates < 1 || h->n * (int64_t)n_replicates >= ((int64_t)1 << 31)) return fail(h, GPF_ERR_INVALID_ARGUMENT, "bad n_replicates");
    const int64_t n_old = h->n, n_new = n_old * n_replicates;
    Bufs old = take_particle_buffers(h);
    set_count(h, n_new);
    if ((s = alloc_particle_buffers(h))) { free_bufs(old); return s; }
    GPF_LAUNCH(k_replicate_anc, dim3(grid_for(h, n_new, 8)), dim3(BLOCK), 0, h->stream, n_new, n_old, (int)n_replicates,
                       (int)(interleaved != 0), 0, h->anc);
    launch_gather_rows_lw(h, h->anc, old.rows[old.cur], old.lw, h->rows[0], h->lw, n_new);     // resize.jl:240-242
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    free_bufs(old);
    HIP_TRY(h, hipGetLastError());
    return GPF_OK;
}

gpf_status gpf_dereplicate(gpf_handle h, int32_t n_replicates, int32_t interleaved, int32_t sample)
{
    gpf_status s = resize_ready(h);
    if (s) return s;
    if (n_replicates < 1 || h->n % n_replicates != 0)
        return fail(h, GPF_ERR_INVALID_ARGUMENT, "the number of particles must be a multiple of n_replicates");   // resize.jl:270
    const int64_t n_old = h->n, n_new = n_old / n_replicates;
    Bufs old = take_particle_buffers(h);
    set_count(h, n_new);
    if ((s = alloc_particle_buffers(h))) { free_bufs(old); return s; }
    const int grid = grid_for(h, n_new, 8);
    if (sample) {                                                                                // resize.jl:281-293
        GPF_LAUNCH(k_dereplicate_sample, dim3(grid), dim3(BLOCK), 0, h->stream, old.lw, n_new, n_old, (int)n_replicates,
                           (int)(interleaved != 0), h->cfg.seed, h->epoch, fix_K(n_replicates), log_((double)n_replicates), h->anc, h->lw);
        launch_gather_rows_lw(h, h->anc, old.rows[old.cur], old.lw, h->rows[0], nullptr, n_new);
        h->epoch += 1;
    } else {                                                                                     // :keepfirst, resize.jl:274-279
        GPF_LAUNCH(k_replicate_anc, dim3(grid), dim3(BLOCK), 0, h->stream, n_new, n_old, (int)n_replicates,
                           (int)(interleaved != 0), 1, h->anc);
        launch_gather_rows_lw(h, h->anc, old.rows[old.cur], old.lw, h->rows[0], h->lw, n_new);
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    free_bufs(old);
    HIP_TRY(h, hipGetLastError());
    return GPF_OK;
}

// pf_coalesce! (resize.jl:309-334) -- gpf.h gpf_coalesce.  Four passes (gpf_k_coalesce.hpp) and one host read of the group count.
} // extern "C"
namespace gpfh {
// device scratch of ONE call (hash table, slots, tile counts / the observation history) is a local Dev<T>: freed on every return path -- hipFree
// waits for the device, so no kernel of the call still reads it -- and never kept on the handle (46 MB at n = 10^6)
static size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
template <int W>
void launch_coal(gpf_filter* h, const CoalArgs& a, int stage, double log_ratio = 0.0)
{
    const unsigned nt = (unsigned)a.ntiles;
    if (stage == 0) {
        GPF_LAUNCH((k_coal_insert<W>), dim3(grid_for(h, a.n, 8)), dim3(BLOCK), 0, h->stream, a);
        GPF_LAUNCH(k_coal_sum, dim3(nt), dim3(BLOCK), 0, h->stream, a);
        GPF_LAUNCH(k_coal_scan, dim3(1), dim3(BLOCK), 0, h->stream, a);
    } else {
        GPF_LAUNCH((k_coal_emit<W>), dim3(nt), dim3(BLOCK), 0, h->stream, a, log_ratio, h->rows[0], h->lw, h->anc);
    }
}
static void launch_coal_w(gpf_filter* h, const CoalArgs& a, int stage, double log_ratio = 0.0)
{
    DISPATCH_W(h, (launch_coal<WW>(h, a, stage, log_ratio)));
}
template <int M, bool KEEP, bool PROP>
void launch_introduce(gpf_filter* h, uint64_t seed, const double* obs, int T, int64_t n_old, int64_t n_add)
{
    using Mo = Model<M>;
    constexpr int Wc = row_width(Mo::D, KEEP);
    if constexpr (PROP && !Mo::HAS_PROPOSAL) { (void)h; (void)seed; (void)obs; (void)T; (void)n_old; (void)n_add; return; }
    else GPF_LAUNCH((k_introduce<M, Wc, KEEP, PROP>), dim3(grid_for(h, n_add, 8)), dim3(BLOCK), 0, h->stream, h->args, seed, obs, T, n_old, n_add,
                    h->rows[0], h->lw, h->anc);
}
} // namespace gpfh
extern "C" {

gpf_status gpf_coalesce(gpf_handle h, uint64_t key_mask, int64_t* n_out)
{
    if (!h) return fail(nullptr, GPF_ERR_INVALID_ARGUMENT, "null handle");
    const int ncols = h->cfg.keep_prev ? 2 * h->d : h->d;          // the padding column of odd widths is never part of the key
    const uint64_t all = ((uint64_t)1 << ncols) - 1;
    if (key_mask & ~all) return fail(h, GPF_ERR_INVALID_ARGUMENT, "coalesce: the key names a column beyond the " + std::to_string(ncols) + " state columns");
    gpf_status s = resize_ready(h, false);
    if (s) return s;
    const int64_t n = h->n;
    uint64_t T = 64;                                              // T <= 2^32 (n < 2^31): slots fit in uint32
    while (T < 2 * (uint64_t)n) T <<= 1;
    const int64_t ntl = (n + COAL_TILE - 1) / COAL_TILE;
    const size_t b_claim = align256(T * 4), b_gm = align256(T * 16), b_slot = align256((size_t)n * 4), b_tile = align256((size_t)ntl * 4);
    Dev<char> scr;
    if ((s = scr.alloc(h, b_claim + b_gm + b_slot + 2 * b_tile + 256))) return s;
    char* p = scr;
    CoalArgs a{};
    a.rows = h->rows[h->cur]; a.lw = h->lw; a.n = n; a.mask = (uint32_t)(key_mask ? key_mask : all);
    a.claim = reinterpret_cast<uint32_t*>(p); p += b_claim;
    a.gm = reinterpret_cast<unsigned long long*>(p); p += b_gm;
    a.slot_of = reinterpret_cast<uint32_t*>(p); p += b_slot;
    a.tile_cnt = reinterpret_cast<uint32_t*>(p); p += b_tile;
    a.tile_off = reinterpret_cast<uint32_t*>(p); p += b_tile;
    a.misc = reinterpret_cast<unsigned long long*>(p);
    a.tmask = T - 1; a.K = fix_K(n); a.ntiles = ntl;
    HIP_TRY(h, hipMemsetAsync(a.claim, 0xff, T * 4, h->stream));
    HIP_TRY(h, hipMemsetAsync(a.gm, 0, T * 16, h->stream));
    HIP_TRY(h, hipMemsetAsync(a.misc, 0, 2 * sizeof(unsigned long long), h->stream));
    launch_coal_w(h, a, 0);
    unsigned long long misc[2] = {0, 0};
    HIP_TRY(h, hipMemcpyAsync(misc, a.misc, sizeof(misc), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipGetLastError());
    if (misc[0]) return fail(h, GPF_ERR_INVALID_WEIGHTS, "Invalid weights.");     // NaN / +Inf: nothing changed, views stay valid
    h->generation += 1;                                                           // views of this filter become stale
    const int64_t n_new = (int64_t)misc[1];
    const double log_ratio = log_((double)n_new) - log_((double)n);               // log(n_particles) - log(n_old), resize.jl:326
    Bufs old = take_particle_buffers(h);
    set_count(h, n_new);
    if ((s = alloc_particle_buffers(h))) { free_bufs(old); return s; }
    a.rows = old.rows[old.cur]; a.lw = old.lw;
    launch_coal_w(h, a, 1, log_ratio);
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    free_bufs(old);
    HIP_TRY(h, hipGetLastError());
    if (n_out) *n_out = n_new;
    return GPF_OK;
}

// pf_introduce! (resize.jl:351-421) -- gpf.h gpf_introduce.  One k_introduce launch for the whole history.
gpf_status gpf_introduce(gpf_handle h, const double* obs, int32_t n_obs, int32_t n_steps, int64_t n_particles, int32_t proposal)
{
    if (!h) return fail(nullptr, GPF_ERR_INVALID_ARGUMENT, "null handle");
    if (gpf_status b = bp_refused(h, "gpf_introduce")) return b;
    if (n_steps < 1 || !obs) return fail(h, GPF_ERR_INVALID_ARGUMENT, "introduce: need observations of at least one step");
    if (n_obs != model_obs_dim(h->cfg.model))
        return fail(h, GPF_ERR_INVALID_ARGUMENT, "this model takes " + std::to_string(model_obs_dim(h->cfg.model)) + " observation values per step");
    if (n_particles < 1 || h->n + n_particles >= ((int64_t)1 << 31)) return fail(h, GPF_ERR_INVALID_ARGUMENT, "introduce: bad n_particles");
    if (proposal != 0 && !(proposal_valid(h, proposal) && model_caps(h).proposal)) return fail(h, GPF_ERR_INVALID_ARGUMENT, "unknown proposal id for this model");
    gpf_status s = resize_ready(h);
    if (s) return s;
    const int64_t n_old = h->n;
    std::vector<double> hobs((size_t)n_steps * MAX_OBS, 0.0);
    for (int32_t e = 0; e < n_steps; ++e)
        for (int k = 0; k < n_obs; ++k) hobs[(size_t)e * MAX_OBS + k] = obs[(size_t)e * n_obs + k];
    Dev<double> scr;
    if ((s = scr.alloc(h, hobs.size()))) return s;
    double* dobs = scr;
    HIP_TRY(h, hipMemcpyAsync(dobs, hobs.data(), hobs.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    const uint64_t seed = intro_seed(h->cfg.seed, h->epoch);
    Bufs old = take_particle_buffers(h);
    set_count(h, n_old + n_particles);
    if ((s = alloc_particle_buffers(h))) { free_bufs(old); return s; }
    HIP_TRY(h, hipMemcpyAsync(h->rows[0], old.rows[old.cur], (size_t)n_old * h->W * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(h->anc, old.anc, (size_t)n_old * sizeof(int32_t), hipMemcpyDeviceToDevice, h->stream));
    GPF_LAUNCH(k_intro_old, dim3(grid_for(h, n_old, 8)), dim3(BLOCK), 0, h->stream, old.lw, h->sc.p, n_old, h->lw);
    HIP_TRY(h, hipMemsetAsync(reinterpret_cast<char*>(h->sc.p) + offsetof(Scalars, lml_est), 0, sizeof(double), h->stream));   // log_ml_est = 0
    bool_dispatch(h->cfg.keep_prev != 0, proposal != 0, [&](auto KEEP, auto PROP) {
        DISPATCH_MODEL(h, (launch_introduce<MM, KEEP, PROP>(h, seed, dobs, n_steps, n_old, n_particles)));
    });
    HIP_TRY(h, hipStreamSynchronize(h->stream));                 // (the old buffers and the host copy of the history are read above)
    free_bufs(old);
    HIP_TRY(h, hipGetLastError());
    h->epoch += 1;
    return GPF_OK;
}

// =================================================================================== trajectory store
gpf_status gpf_history_enable(gpf_handle h, int32_t max_steps)
{
    if (!h) return fail(nullptr, GPF_ERR_INVALID_ARGUMENT, "null handle");
    if (max_steps < 1) return fail(h, GPF_ERR_INVALID_ARGUMENT, "max_steps < 1");
    if (h->cfg.n_global != h->n) return fail(h, GPF_ERR_STATE, "the trajectory store is not available for sharded filters");
    if (h->initialized) return fail(h, GPF_ERR_STATE, "enable the trajectory store before gpf_initialize");
    h->hist_on = true; h->hist_blocks = false; h->hist_weights = false; h->hist_cap = max_steps;
    h->hist_dev_maps.reset(); h->hist_dev_x.reset();
    gpf_status s = h->hist_dev_maps.alloc(h, (size_t)max_steps);
    return s ? s : h->hist_dev_x.alloc(h, (size_t)max_steps);
}

// the block-wise store: the same store, fed by the block-wise calls as well (gpf.h)
gpf_status gpf_history_enable_blocks(gpf_handle h, int32_t max_steps)
{
    gpf_status s = gpf_history_enable(h, max_steps);
    if (s) return s;
    h->hist_blocks = true;
    return GPF_OK;
}

// ... plus the records of a backward pass: every step's log-weights and per-block observation rows (gpf.h)
gpf_status gpf_history_enable_blocks_weights(gpf_handle h, int32_t max_steps)
{
    gpf_status s = gpf_history_enable_blocks(h, max_steps);
    if (s) return s;
    h->hist_dev_lw.reset(); h->hist_dev_obs.reset();
    if ((s = h->hist_dev_lw.alloc(h, (size_t)max_steps)) || (s = h->hist_dev_obs.alloc(h, (size_t)max_steps))) return s;
    h->hist_weights = true;
    return GPF_OK;
}

gpf_status gpf_history_steps(gpf_handle h, int32_t* n_steps)
{
    if (!h || !n_steps) return fail(h, GPF_ERR_INVALID_ARGUMENT, "null argument");
    *n_steps = h->hist_on ? (int32_t)h->hist_x.size() : 0;
    return GPF_OK;
}

// column `column` of time step `step` (1-based, like the t of the Julia address t => :name) into h->dtmp
static gpf_status history_values(gpf_handle h, int32_t step, int32_t column)
{
    gpf_status s = check_ready(h);
    if (s) return s;
    if (!h->hist_on) return fail(h, GPF_ERR_STATE, "trajectory store not enabled (gpf_history_enable)");
    const int T = (int)h->hist_x.size();
    if (step < 1 || step > T || column < 0 || column >= h->d) return fail(h, GPF_ERR_INVALID_ARGUMENT, "bad step/column");
    if ((s = hist_snapshot(h))) return s;                         // the current step, in its current order
    // maps of steps T, T-1, ..., step+1 (0-based indices T-1 ... step), applied in that order
    std::vector<const int32_t*> maps;
    for (int q = T - 1; q >= step; --q) maps.push_back(h->hist_map[q]);
    if (!maps.empty())
        HIP_TRY(h, hipMemcpyAsync(h->hist_dev_maps, maps.data(), maps.size() * sizeof(int32_t*), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));                   // `maps` is a host temporary
    GPF_LAUNCH(k_hist_column, dim3(grid_for(h, h->n, 8)), dim3(BLOCK), 0, h->stream, h->hist_dev_maps.p, (int)maps.size(),
                       h->hist_x[step - 1].p, h->d, (int)column, h->n, h->dtmp);
    HIP_TRY(h, hipGetLastError());
    return GPF_OK;
}

gpf_status gpf_history_column(gpf_handle h, int32_t step, int32_t column, double* out, int64_t n)
{
    if (!h) return fail(nullptr, GPF_ERR_INVALID_ARGUMENT, "null handle");
    if (!out || n != h->n) return fail(h, GPF_ERR_INVALID_ARGUMENT, "bad output array");
    gpf_status s = history_values(h, step, column);
    if (s) return s;
    return copy_out(h, h->dtmp, out, (size_t)n * sizeof(double));
}

static gpf_status history_stat(gpf_handle h, int32_t step, int32_t column, double* out, bool variance)
{
    if (!h || !out) return fail(h, GPF_ERR_INVALID_ARGUMENT, "null argument");
    gpf_status s = history_values(h, step, column);
    if (s) return s;
    if ((s = ensure_raw(h))) return s;
    if ((s = weighted_tree_sum(h, h->dtmp, 1, 0, 1, nullptr, 0.0, h->dscal))) return s;
    if (variance && (s = weighted_tree_sum(h, h->dtmp, 1, 0, 2, h->dscal, 0.0, h->dscal + 1))) return s;
    double tmp[2];
    if ((s = copy_out(h, h->dscal, tmp, sizeof(tmp)))) return s;
    *out = variance ? tmp[1] : tmp[0];
    return GPF_OK;
}
// proportionmap(state, addr)[value] (statistics.jl:91-101): normalised weight of the particles whose column equals `value`;
// step = 0: the current step's column, step >= 1: a past choice along the ancestry (trajectory store)
gpf_status gpf_proportion(gpf_handle h, int32_t step, int32_t column, double value, double* out)
{
    if (!h || !out) return fail(h, GPF_ERR_INVALID_ARGUMENT, "null argument");
    gpf_status s;
    if (step > 0) { if ((s = history_values(h, step, column))) return s; }
    else {
        if ((s = check_ready(h))) return s;
        if (column < 0 || column >= h->W) return fail(h, GPF_ERR_INVALID_ARGUMENT, "bad column");
        if ((s = materialize(h))) return s;
        GPF_LAUNCH(k_extract_column, dim3(grid_for(h, h->n, 8)), dim3(BLOCK), 0, h->stream, h->rows[h->cur], h->W, column, h->n, h->dtmp);
    }
    if ((s = ensure_raw(h))) return s;
    if ((s = weighted_tree_sum(h, h->dtmp, 1, 0, 3, nullptr, value, h->dscal))) return s;
    return copy_out(h, h->dscal, out, sizeof(double));
}

// ---- past choices per block (gpf.h gpf_block_history_moments / _proportion): the block-wise store queried block by block, one launch
} // extern "C"
namespace gpfh {
// The preamble of a query of the block-wise store, in ONE order ("the gate of the block-wise calls"): the gate, the query's own arguments,
// the step range (which brings the filter up to date), the 2^31 limits, the recorded block sizes, the device tables.  All but the tables change nothing.
// the gate of the queries; block_size comes back clamped.  needs_weights: the queries that read the store's weight records and evaluate the transition density
static gpf_status block_store_gate(gpf_handle h, int64_t& block_size, const char* who, bool needs_weights = false)
{
    gpf_status s = block_gate(h, block_size, who, GATE_SIZE | GATE_CLAMP_STORE | GATE_MAX);
    if (s) return s;
    if (!h->hist_on || !h->hist_blocks)
        return fail(h, GPF_ERR_STATE, std::string(who) + " needs the block-wise trajectory store (gpf_history_enable_blocks before gpf_initialize_blocks)");
    if (h->d != 1 && h->d != 2 && h->d != 4) return fail(h, GPF_ERR_STATE, "latent dimension");
    if (!needs_weights) return GPF_OK;
    if (!h->hist_weights)
        return fail(h, GPF_ERR_STATE, std::string(who) + " needs the store's weight records (gpf_history_enable_blocks_weights before gpf_initialize_blocks)");
    return block_gate(h, block_size, who, GATE_PARAMS);
}
// the steps a query walks, 1 <= step_lo <= step_hi <= T, on a filter brought up to date
struct StoreSteps { int T; int64_t nblocks, n_steps; };
static gpf_status block_store_steps(gpf_handle h, int64_t block_size, int32_t step_lo, int32_t step_hi, const char* who, StoreSteps& r)
{
    gpf_status s = check_ready(h);
    if (s) return s;
    r.T = (int)h->hist_x.size();
    if (step_lo < 1 || step_hi < step_lo || step_hi > r.T) return fail(h, GPF_ERR_INVALID_ARGUMENT, std::string(who) + ": need 1 <= step_lo <= step_hi <= gpf_history_steps");
    r.nblocks = (h->n + block_size - 1) / block_size; r.n_steps = step_hi - step_lo + 1;
    return GPF_OK;
}
// what the samplers return stays below 2^31 draws and cells: *draws = n_blocks * n_samples
// (nblocks <= n < 2^31, n_samples < 2^31, n_steps d < 2^31: no product below overflows 64 bits before it is compared)
static gpf_status block_store_draws(gpf_handle h, const StoreSteps& r, int32_t n_samples, const char* who, int64_t* draws)
{
    const int64_t lim = (int64_t)1 << 31, row = r.n_steps * h->d;
    *draws = r.nblocks * n_samples;
    if (*draws >= lim || row >= lim || *draws >= (lim + row - 1) / row)
        return fail(h, GPF_ERR_INVALID_ARGUMENT, std::string(who) + ": n_blocks * n_samples and n_blocks * n_samples * n_steps * dim must stay below 2^31");
    return GPF_OK;
}
// every walked step above step_lo reads the observation rows it was entered with, by the particle's block: a block-wise step of this block size
static gpf_status block_store_sizes(gpf_handle h, int64_t block_size, int T, int32_t step_lo, const char* who)
{
    for (int q = T - 1; q >= step_lo; --q) {
        if (h->hist_bsize[q] == 0)
            return fail(h, GPF_ERR_STATE, std::string(who) + ": step " + std::to_string(q + 1) + " was entered by a whole-filter call (no per-block observations were recorded)");
        if (h->hist_bsize[q] != block_size)
            return fail(h, GPF_ERR_INVALID_ARGUMENT, std::string(who) + ": block_size " + std::to_string(block_size) + " differs from the " +
                        std::to_string(h->hist_bsize[q]) + " step " + std::to_string(q + 1) + " was entered with");
    }
    return GPF_OK;
}
// whatever is deferred becomes state (the current step is snapshotted, in its current order); then the device tables, indexed by the 0-based step: the
// snapshots and the composed ancestor maps (nullptr: a step without a resample), with_weights: the log-weights and the observation rows as well
static gpf_status block_store_tables(gpf_handle h, bool with_weights)
{
    gpf_status s = hist_snapshot(h);
    if (s) return s;
    std::vector<const void*> host[4];                             // (host temporaries until the synchronisation)
    auto put = [&](int k, void* dev, const auto& v) {
        host[k].assign(v.begin(), v.end());
        return hipMemcpyAsync(dev, host[k].data(), host[k].size() * sizeof(void*), hipMemcpyHostToDevice, h->stream);
    };
    HIP_TRY(h, put(0, h->hist_dev_maps, h->hist_map));
    HIP_TRY(h, put(1, h->hist_dev_x, h->hist_x));
    if (with_weights) { HIP_TRY(h, put(2, h->hist_dev_lw, h->hist_lw)); HIP_TRY(h, put(3, h->hist_dev_obs, h->hist_obs)); }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return GPF_OK;
}
// the inputs of block_store_walk (SmoothArgs and PairArgs): the tables of block_store_tables(h, true) and the walked steps, 0-based
static void block_store_walk_args(gpf_handle h, const StoreSteps& r, int32_t step_lo, int32_t step_hi, int64_t block_size, StoreWalkArgs& a)
{
    a.maps = h->hist_dev_maps; a.hx = h->hist_dev_x; a.hlw = h->hist_dev_lw; a.hobs = h->hist_dev_obs; a.lw = h->lw;
    a.T = r.T; a.lo0 = step_lo - 1; a.hi0 = step_hi - 1;
    a.n = h->n; a.nb = block_size; a.nblocks = r.nblocks;
}
// device scratch of one query for an output that was asked for (up to 16 GB of trajectories are nothing to keep on a handle)
template <class T>
static gpf_status block_store_scratch(gpf_handle h, Dev<T>& c, const void* wanted, size_t bytes)
{
    return wanted ? c.alloc(h, bytes / sizeof(T)) : GPF_OK;
}
// what both estimate queries do once the gate and their own arguments have passed: the current step is snapshotted and the maps of the steps
// T, T-1, ..., step+1 go to h->hist_dev_maps (as history_values): *n_maps of them
static gpf_status block_hist_prepare(gpf_handle h, int32_t step, int* n_maps)
{
    gpf_status s = check_ready(h);
    if (s) return s;
    const int T = (int)h->hist_x.size();
    if (step < 1 || step > T) return fail(h, GPF_ERR_INVALID_ARGUMENT, "bad step");
    if ((s = hist_snapshot(h))) return s;                         // the current step, in its current order
    std::vector<const int32_t*> maps;
    for (int q = T - 1; q >= step; --q) maps.push_back(h->hist_map[q]);
    if (!maps.empty())
        HIP_TRY(h, hipMemcpyAsync(h->hist_dev_maps, maps.data(), maps.size() * sizeof(int32_t*), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));                   // `maps` is a host temporary
    *n_maps = (int)maps.size();
    return GPF_OK;
}
template <int D>
void launch_block_hist_moments(gpf_filter* h, int n_maps, const double* hx, int64_t nb, int64_t nblocks, int want_var, double* mean, double* var)
{
    team_dispatch(nb, nblocks, [&](auto TEAM, auto ITEMS, dim3 grid) {
        GPF_LAUNCH((k_block_hist_moments<D, TEAM, ITEMS>), grid, dim3(BLOCK), 0, h->stream, h->hist_dev_maps.p, n_maps, hx, h->lw, h->n, nb, nblocks, want_var, mean, var);
    });
}
} // namespace gpfh
extern "C" {
// for b in blocks: [mean(state[b], step => c) for c in latent columns], [var(state[b], step => c) ...]
// (src/statistics.jl:13-14, 48-50 with a past address on sub-states, src/view.jl:35-48) -- gpf.h
gpf_status gpf_block_history_moments(gpf_handle h, int32_t step, int64_t block_size, double* mean_out, double* var_out)
{
    gpf_status s = block_store_gate(h, block_size, "gpf_block_history_moments");
    if (s) return s;
    if (!mean_out && !var_out) return fail(h, GPF_ERR_INVALID_ARGUMENT, "gpf_block_history_moments: both outputs are NULL");
    int n_maps = 0;
    if ((s = block_hist_prepare(h, step, &n_maps))) return s;
    const int64_t nblocks = (h->n + block_size - 1) / block_size;
    const size_t cells = (size_t)nblocks * (size_t)h->d;
    if ((s = block_est_buffer(h, (int64_t)(2 * cells)))) return s;
    double* const mean = h->blk_est; double* const var = h->blk_est + cells;
    const double* hx = h->hist_x[step - 1];
    DISPATCH_D(h, (launch_block_hist_moments<DD>(h, n_maps, hx, block_size, nblocks, var_out ? 1 : 0, mean, var)));
    HIP_TRY(h, hipGetLastError());
    return block_out(h, {{mean, mean_out, cells * sizeof(double)}, {var, var_out, cells * sizeof(double)}});
}
// for b in blocks: proportionmap(state[b], step => column)[values[k]] (src/statistics.jl:91-101 with a past address on sub-states) -- gpf.h
gpf_status gpf_block_history_proportion(gpf_handle h, int32_t step, int64_t block_size, int32_t column, const double* values, int32_t n_values, double* out)
{
    gpf_status s = block_store_gate(h, block_size, "gpf_block_history_proportion");
    if (s) return s;
    if (!values || !out) return fail(h, GPF_ERR_INVALID_ARGUMENT, "gpf_block_history_proportion: null values / output");
    if (column < 0 || column >= h->d) return fail(h, GPF_ERR_INVALID_ARGUMENT, "bad column");
    if (n_values < 1 || n_values > BLK_MATCH_MAX) return fail(h, GPF_ERR_INVALID_ARGUMENT, "gpf_block_history_proportion: need 1 <= n_values <= " + std::to_string(BLK_MATCH_MAX));
    int n_maps = 0;
    if ((s = block_hist_prepare(h, step, &n_maps))) return s;
    const int64_t nblocks = (h->n + block_size - 1) / block_size;
    const size_t cells = (size_t)nblocks * (size_t)n_values;
    if ((s = block_est_buffer(h, (int64_t)cells))) return s;
    const BlockMatch mv = make_block_match(values, n_values);
    const double* hx = h->hist_x[step - 1];
    team_dispatch(block_size, nblocks, [&](auto TEAM, auto ITEMS, dim3 grid) {
        GPF_LAUNCH((k_block_hist_proportion<TEAM, ITEMS>), grid, dim3(BLOCK), 0, h->stream, h->hist_dev_maps.p, n_maps, hx, h->d, (int)column, h->lw, h->n, block_size, nblocks, mv, h->blk_est.p);
    });
    HIP_TRY(h, hipGetLastError());
    return block_out(h, {{h->blk_est, out, cells * sizeof(double)}});
}
// ---- whole trajectories per block (gpf.h gpf_block_sample_trajectories): weights, draws, genealogy walk and gather of all blocks in one launch
} // extern "C"
namespace gpfh {
struct TrajLaunch { int T, lo0, hi0; int64_t nb, nblocks; int n_samples; double* traj; int64_t* idx; };
template <int D>
void launch_block_sample_traj(gpf_filter* h, const TrajLaunch& a)
{
    team_dispatch(a.nb, a.nblocks, [&](auto TEAM, auto ITEMS, dim3 grid) {
        GPF_LAUNCH((k_block_sample_traj<D, TEAM, ITEMS>), grid, dim3(BLOCK), 0, h->stream, h->hist_dev_maps.p, h->hist_dev_x.p, a.T, a.lo0, a.hi0, h->lw, h->n, a.nb, a.nblocks,
                   a.n_samples, h->cfg.seed, h->epoch, a.traj, a.idx);
    });
}
} // namespace gpfh
extern "C" {
// for b in blocks; sample_unweighted_traces(state[b], n_samples); end (src/utils.jl:7,189-194 on sub-states, src/view.jl:35-48) -- gpf.h
gpf_status gpf_block_sample_trajectories(gpf_handle h, int64_t block_size, int32_t n_samples, int32_t step_lo, int32_t step_hi,
                                         double* traj_out, int64_t* idx_out)
{
    const char* who = "gpf_block_sample_trajectories";
    gpf_status s = block_store_gate(h, block_size, who);
    if (s) return s;
    if (!traj_out && !idx_out) return fail(h, GPF_ERR_INVALID_ARGUMENT, std::string(who) + ": both outputs are NULL");
    if (n_samples < 1) return fail(h, GPF_ERR_INVALID_ARGUMENT, std::string(who) + ": n_samples < 1");
    StoreSteps r{};
    int64_t draws = 0;
    if ((s = block_store_steps(h, block_size, step_lo, step_hi, who, r)) || (s = block_store_draws(h, r, n_samples, who, &draws))) return s;
    const size_t b_traj = (size_t)draws * (size_t)r.n_steps * (size_t)h->d * sizeof(double), b_idx = (size_t)draws * sizeof(int64_t);
    Dev<double> d_traj; Dev<int64_t> d_idx;                                    // scratch of this call: freed before it returns
    if ((s = block_store_tables(h, false)) || (s = block_store_scratch(h, d_traj, traj_out, b_traj)) || (s = block_store_scratch(h, d_idx, idx_out, b_idx))) return s;
    const TrajLaunch a{r.T, step_lo - 1, step_hi - 1, block_size, r.nblocks, (int)n_samples, d_traj, d_idx};
    DISPATCH_D(h, (launch_block_sample_traj<DD>(h, a)));
    HIP_TRY(h, hipGetLastError());
    if ((s = block_out(h, {{d_traj.p, traj_out, b_traj}, {d_idx.p, idx_out, b_idx}}))) return s;
    h->epoch += 1;                                                // as gpf_sample_unweighted: the draws' slots are not read again
    return GPF_OK;
}
// ---- backward simulation per block (gpf.h gpf_block_backward_sample): the step-T draw and the whole backward pass of all blocks and draws in one launch
} // extern "C"
namespace gpfh {
template <int M>
void launch_block_backward(gpf_filter* h, const BackArgs& a, const AncArgs& x)
{
    team_dispatch(a.nb, a.nblocks, [&](auto TEAM, auto ITEMS, dim3 grid) {
        // (the draws of a block are independent: with few blocks they are dealt to gridDim.y workgroups per block, so that the launch fills the chip)
        grid.y = (unsigned)std::max<int64_t>(1, std::min<int64_t>(a.n_samples, 2048 / std::max<int64_t>(1, (int64_t)grid.x)));
        GPF_LAUNCH((k_block_backward<M, TEAM, ITEMS>), grid, dim3(BLOCK), 0, h->stream, a, x);
    });
}
} // namespace gpfh
extern "C" {
gpf_status gpf_block_backward_sample(gpf_handle h, int64_t block_size, int32_t n_samples, int32_t step_lo, int32_t step_hi,
                                     double* traj_out, int64_t* idx_out)
{
    const char* who = "gpf_block_backward_sample";
    gpf_status s = block_store_gate(h, block_size, who, true);
    if (s) return s;
    if (!traj_out) return fail(h, GPF_ERR_INVALID_ARGUMENT, std::string(who) + ": null trajectory output");
    if (n_samples < 1) return fail(h, GPF_ERR_INVALID_ARGUMENT, std::string(who) + ": n_samples < 1");
    StoreSteps r{};
    int64_t draws = 0;
    if ((s = block_store_steps(h, block_size, step_lo, step_hi, who, r)) || (s = block_store_draws(h, r, n_samples, who, &draws)) ||
        (s = block_store_sizes(h, block_size, r.T, step_lo, who))) return s;
    const size_t b_traj = (size_t)draws * (size_t)r.n_steps * (size_t)h->d * sizeof(double), b_idx = (size_t)draws * (size_t)r.n_steps * sizeof(int64_t);
    Dev<double> d_traj; Dev<int64_t> d_idx;                                    // scratch of this call, as gpf_block_sample_trajectories
    if ((s = block_store_tables(h, true)) || (s = block_store_scratch(h, d_traj, traj_out, b_traj)) || (s = block_store_scratch(h, d_idx, idx_out, b_idx))) return s;
    BackArgs a{};
    a.maps = h->hist_dev_maps; a.hx = h->hist_dev_x; a.hlw = h->hist_dev_lw; a.hobs = h->hist_dev_obs; a.lw = h->lw;
    a.T = r.T; a.lo0 = step_lo - 1; a.hi0 = step_hi - 1; a.n_samples = (int)n_samples;
    a.n = h->n; a.nb = block_size; a.nblocks = r.nblocks; a.seed = h->cfg.seed; a.epoch = h->epoch;
    a.traj = d_traj; a.idx = d_idx;
    const AncArgs x = anc_args(h);
    DISPATCH_MODEL(h, (launch_block_backward<MM>(h, a, x)));
    HIP_TRY(h, hipGetLastError());
    if ((s = block_out(h, {{d_traj.p, traj_out, b_traj}, {d_idx.p, idx_out, b_idx}}))) return s;
    h->epoch += (uint32_t)(r.T - step_lo + 1);                    // one epoch for the step-T draw and one per backward step down to step_lo
    return GPF_OK;
}
// ---- marginal smoothing per block (gpf.h gpf_block_smooth): the smoothing weights and moments of all blocks and steps in one launch.  The kernels are
// instantiated in a translation unit of their own (libgpf_smooth.hip): this unit's device code is what it was
gpf_status gpf_block_smooth(gpf_handle h, int64_t block_size, int32_t step_lo, int32_t step_hi,
                            double* mean_out, double* var_out, double* weights_out, int64_t* blocks_out)
{
    const char* who = "gpf_block_smooth";
    gpf_status s = block_store_gate(h, block_size, who, true);
    if (s) return s;
    if (!mean_out && !var_out && !weights_out && !blocks_out) return fail(h, GPF_ERR_INVALID_ARGUMENT, std::string(who) + ": all outputs are NULL");
    StoreSteps r{};
    if ((s = block_store_steps(h, block_size, step_lo, step_hi, who, r))) return s;
    const int64_t lim = (int64_t)1 << 31, cells = r.nblocks * r.n_steps;
    const int64_t row = std::max<int64_t>(h->d, weights_out ? block_size : 1);   // (nblocks, n_steps, row < 2^31: the product below does not overflow before it is compared)
    if (cells >= lim || cells >= (lim + row - 1) / row)
        return fail(h, GPF_ERR_INVALID_ARGUMENT, std::string(who) + ": n_blocks * n_steps * dim and n_blocks * n_steps * block_size must stay below 2^31");
    if ((s = block_store_sizes(h, block_size, r.T, step_lo, who))) return s;
    const size_t b_mom = (size_t)cells * (size_t)h->d * sizeof(double), b_w = (size_t)cells * (size_t)block_size * sizeof(double), b_c = (size_t)cells * sizeof(int64_t);
    Dev<double> d_mean, d_var, d_w; Dev<int64_t> d_c;                          // scratch of this call, as gpf_block_backward_sample; only what was asked for
    if ((s = block_store_tables(h, true)) || (s = block_store_scratch(h, d_mean, mean_out, b_mom)) || (s = block_store_scratch(h, d_var, var_out, b_mom)) ||
        (s = block_store_scratch(h, d_w, weights_out, b_w)) || (s = block_store_scratch(h, d_c, blocks_out, b_c))) return s;
    SmoothArgs a{};
    block_store_walk_args(h, r, step_lo, step_hi, block_size, a);
    a.mean = d_mean; a.var = d_var;
    a.wout = d_w; a.blocks = d_c;
    launch_block_smooth(h, a, anc_args(h));
    HIP_TRY(h, hipGetLastError());
    // (nothing was drawn: the epoch stays)
    return block_out(h, {{d_mean.p, mean_out, b_mom}, {d_var.p, var_out, b_mom}, {d_w.p, weights_out, b_w}, {d_c.p, blocks_out, b_c}});
}
// ---- pairwise smoothing per block (gpf.h gpf_block_smooth_pairs): the smoothed mean, second moments and lag-one cross moments of all blocks and steps
// in one launch; gpf_block_smooth's gate, checks and walk, and like it instantiated in a translation unit of its own (libgpf_pairs.hip)
gpf_status gpf_block_smooth_pairs(gpf_handle h, int64_t block_size, int32_t step_lo, int32_t step_hi,
                                  double* mean_out, double* second_out, double* cross_out, int64_t* blocks_out)
{
    const char* who = "gpf_block_smooth_pairs";
    gpf_status s = block_store_gate(h, block_size, who, true);
    if (s) return s;
    if (!mean_out && !second_out && !cross_out && !blocks_out) return fail(h, GPF_ERR_INVALID_ARGUMENT, std::string(who) + ": all outputs are NULL");
    StoreSteps r{};
    if ((s = block_store_steps(h, block_size, step_lo, step_hi, who, r))) return s;
    if (cross_out && step_lo == step_hi) return fail(h, GPF_ERR_INVALID_ARGUMENT, std::string(who) + ": cross_out needs two steps at least (no pair in the range)");
    const int64_t lim = (int64_t)1 << 31, cells = r.nblocks * r.n_steps, dd = (int64_t)h->d * h->d;   // (nblocks, n_steps, dd < 2^31: as gpf_block_smooth)
    if (cells >= lim || cells >= (lim + dd - 1) / dd)
        return fail(h, GPF_ERR_INVALID_ARGUMENT, std::string(who) + ": n_blocks * n_steps * dim * dim must stay below 2^31");
    if ((s = block_store_sizes(h, block_size, r.T, step_lo, who))) return s;
    const size_t b_mean = (size_t)cells * (size_t)h->d * sizeof(double), b_sec = (size_t)cells * (size_t)dd * sizeof(double),
                 b_cross = (size_t)(r.nblocks * (r.n_steps - 1)) * (size_t)dd * sizeof(double), b_c = (size_t)cells * sizeof(int64_t);
    Dev<double> d_mean, d_sec, d_cross; Dev<int64_t> d_c;                      // scratch of this call, as gpf_block_smooth; only what was asked for
    if ((s = block_store_tables(h, true)) || (s = block_store_scratch(h, d_mean, mean_out, b_mean)) || (s = block_store_scratch(h, d_sec, second_out, b_sec)) ||
        (s = block_store_scratch(h, d_cross, cross_out, b_cross)) || (s = block_store_scratch(h, d_c, blocks_out, b_c))) return s;
    PairArgs a{};
    block_store_walk_args(h, r, step_lo, step_hi, block_size, a);
    a.mean = d_mean; a.second = d_sec;
    a.cross = d_cross; a.blocks = d_c;
    launch_block_pairs(h, a, anc_args(h));
    HIP_TRY(h, hipGetLastError());
    // (nothing was drawn: the epoch stays)
    return block_out(h, {{d_mean.p, mean_out, b_mean}, {d_sec.p, second_out, b_sec}, {d_cross.p, cross_out, b_cross}, {d_c.p, blocks_out, b_c}});
}
// ---- the most probable path per block (gpf.h gpf_block_map_path): max-plus dynamic programming over the store's grid and the trace, all
// blocks and steps in one launch; gpf_block_smooth's gate and checks, and like it instantiated in a translation unit of its own (libgpf_map.hip).  The DP
// always walks T .. 1 whatever the range written, so every step -- step 1 too, whose observation row the node score and the prior term read -- must have
// been entered by a block-wise call of this block size
gpf_status gpf_block_map_path(gpf_handle h, int64_t block_size, int32_t step_lo, int32_t step_hi, double* path_out, int64_t* idx_out, double* logp_out)
{
    const char* who = "gpf_block_map_path";
    gpf_status s = block_store_gate(h, block_size, who, true);
    if (s) return s;
    if (!path_out && !idx_out && !logp_out) return fail(h, GPF_ERR_INVALID_ARGUMENT, std::string(who) + ": all outputs are NULL");
    StoreSteps r{};
    if ((s = block_store_steps(h, block_size, step_lo, step_hi, who, r))) return s;
    const int64_t lim = (int64_t)1 << 31, cells = r.nblocks * r.n_steps;   // (nblocks, n_steps, d < 2^31: as gpf_block_smooth)
    if (cells >= lim || cells >= (lim + h->d - 1) / h->d)
        return fail(h, GPF_ERR_INVALID_ARGUMENT, std::string(who) + ": n_blocks * n_steps * dim must stay below 2^31");
    if ((s = block_store_sizes(h, block_size, r.T, 0, who))) return s;
    const size_t b_path = (size_t)cells * (size_t)h->d * sizeof(double), b_idx = (size_t)cells * sizeof(int64_t), b_lp = (size_t)r.nblocks * sizeof(double);
    // the back-pointers (2 bytes per particle and step, rows padded to 16 bytes) and the lineage blocks: scratch of this call like the outputs' device
    // copies -- 198 MB at 10^4 blocks of 100 and T = 100 are nothing to keep on a handle; hipFree on return waits for the launch
    const int64_t bsp = (block_size + 7) / 8 * 8;
    const size_t b_ptr = (size_t)std::max(r.T - 1, 1) * (size_t)r.nblocks * (size_t)bsp * sizeof(uint16_t), b_lin = (size_t)r.nblocks * (size_t)r.T * sizeof(int32_t);
    Dev<double> d_path, d_lp; Dev<int64_t> d_idx; Dev<uint16_t> d_ptr; Dev<int32_t> d_lin;
    if ((s = block_store_tables(h, true)) || (s = block_store_scratch(h, d_path, path_out, b_path)) || (s = block_store_scratch(h, d_idx, idx_out, b_idx)) ||
        (s = block_store_scratch(h, d_lp, logp_out, b_lp)) || (s = block_store_scratch(h, d_ptr, h, b_ptr)) || (s = block_store_scratch(h, d_lin, h, b_lin))) return s;
    MapArgs a{};
    block_store_walk_args(h, r, step_lo, step_hi, block_size, a);
    a.path = d_path; a.idx = d_idx; a.logp = d_lp;
    a.ptr = d_ptr; a.lin = d_lin; a.bsp = bsp;
    launch_block_map(h, a, anc_args(h));
    HIP_TRY(h, hipGetLastError());
    // (nothing was drawn: the epoch stays)
    return block_out(h, {{d_path.p, path_out, b_path}, {d_idx.p, idx_out, b_idx}, {d_lp.p, logp_out, b_lp}});
}
// ---- forward-only smoothing per block (gpf.h gpf_forward_enable_blocks / gpf_block_forward_moments): the additive smoothing functionals
// of particle EM after every step, from one generation of records.  The records, the hooks of the block-wise calls and the kernels' instantiations live in
// a translation unit of their own (libgpf_forward.hip)
gpf_status gpf_forward_enable_blocks(gpf_handle h)
{
    if (!h) return fail(nullptr, GPF_ERR_INVALID_ARGUMENT, "null handle");
    if (h->parent) return fail(h, GPF_ERR_STATE, "gpf_forward_enable_blocks on a sub-state view: call it on the filter");
    if (h->cfg.n_global != h->n || h->comm) return fail(h, GPF_ERR_STATE, "forward smoothing per block is not available for sharded filters");
    if (h->initialized) return fail(h, GPF_ERR_STATE, "enable forward smoothing per block before gpf_initialize_blocks");
    if (h->hist_on && !h->hist_blocks) return fail(h, GPF_ERR_STATE, "forward smoothing per block follows the block-wise calls: the plain trajectory store refuses them");
    if (!h->views.empty()) return fail(h, GPF_ERR_STATE, "forward smoothing per block on a filter with sub-state views");
    h->fwd_on = true; h->fwd_bsize = 0; h->fwd_steps = 0;
    return GPF_OK;
}
gpf_status gpf_block_forward_moments(gpf_handle h, int64_t block_size, double* sum_out, double* second_out, double* cross_out, double* first_out,
                                     double* first2_out, double* last2_out, int32_t* n_steps_out)
{
    const char* who = "gpf_block_forward_moments";
    if (!h) return fail(nullptr, GPF_ERR_INVALID_ARGUMENT, "null handle");
    if (!h->fwd_on) return fail(h, GPF_ERR_STATE, std::string(who) + " needs forward smoothing per block (gpf_forward_enable_blocks before gpf_initialize_blocks)");
    if (!h->initialized || h->fwd_steps < 1) return fail(h, GPF_ERR_STATE, std::string(who) + ": nothing is initialised (gpf_initialize_blocks)");
    gpf_status s = block_gate(h, block_size, who, GATE_SIZE | GATE_CLAMP | GATE_FWD | GATE_PARAMS);   // (the rows of the per-block parameters are read by block)
    if (s) return s;
    if (!sum_out && !second_out && !cross_out && !first_out && !first2_out && !last2_out && !n_steps_out)
        return fail(h, GPF_ERR_INVALID_ARGUMENT, std::string(who) + ": all outputs are NULL");
    if ((s = check_ready(h)) || (s = materialize(h))) return s;
    const int d = h->d, F = fwd_F(d), tri = d * (d + 1) / 2, row = F + d * d;
    const int64_t nblocks = (h->n + block_size - 1) / block_size;
    if ((s = block_est_buffer(h, nblocks * row))) return s;
    // the current step's statistics as a close would form them, into the half of the ping-pong the close writes: nothing is committed, the close recomputes
    if ((s = fwd_form(h))) return s;
    launch_block_forward_reduce(h, h->fwd_T[1 - h->fwd_cur], h->blk_est);
    HIP_TRY(h, hipGetLastError());
    std::vector<double> host((size_t)(nblocks * row));
    if ((s = block_out(h, {{h->blk_est, host.data(), host.size() * sizeof(double)}}))) return s;
    // [sum | second, upper triangle | cross | first | first2, upper triangle | last2] per block -> the caller's arrays, triangles mirrored
    auto vec = [&](double* out, int off) {
        if (out) for (int64_t b = 0; b < nblocks; ++b) for (int a = 0; a < d; ++a) out[b * d + a] = host[(size_t)(b * row + off + a)];
    };
    auto full = [&](double* out, int off) {
        if (out) for (int64_t b = 0; b < nblocks; ++b) for (int k = 0; k < d * d; ++k) out[b * d * d + k] = host[(size_t)(b * row + off + k)];
    };
    auto mirrored = [&](double* out, int off) {
        if (!out) return;
        for (int64_t b = 0; b < nblocks; ++b) {
            int t = 0;
            for (int a = 0; a < d; ++a)
                for (int c = a; c < d; ++c, ++t) out[(b * d + a) * d + c] = out[(b * d + c) * d + a] = host[(size_t)(b * row + off + t)];
        }
    };
    vec(sum_out, 0); mirrored(second_out, d); full(cross_out, d + tri); vec(first_out, d + tri + d * d); mirrored(first2_out, d + tri + d * d + d); full(last2_out, F);
    if (n_steps_out) *n_steps_out = h->fwd_steps;
    return GPF_OK;
}
// ---- checkpoint / resume: everything a filter needs to continue bit for bit -- the population, its log-weights and parents, the log-ML
// estimate, the RNG epoch, the latest observation and strata -- as ONE host blob; loads into a handle created with the same gpf_config
namespace {
struct CkptHeader {
    uint64_t magic; int32_t version, model, keep_prev, W, n_params, has_prev, n_strata, interleaved;
    int64_t n, n_global, gid0; uint64_t seed; uint32_t epoch, pad;
    double lml_est, logK;
    double params[MAX_PARAMS], obs[MAX_OBS], strata[MAX_STRATA], q[4];
};
constexpr uint64_t CKPT_MAGIC = 0x4750465f434b5054ull;          // "GPF_CKPT"
int64_t ckpt_bytes(const gpf_filter* h) { return (int64_t)sizeof(CkptHeader) + h->n * h->W * 8 + h->n * 8 + ((h->n * 4 + 7) & ~(int64_t)7); }
gpf_status ckpt_ready(gpf_filter* h)
{
    if (!h) return fail(nullptr, GPF_ERR_INVALID_ARGUMENT, "null handle");
    if (h->parent) return fail(h, GPF_ERR_STATE, "checkpoints are taken of whole filters, not of sub-state views");
    return GPF_OK;
}
} // namespace
gpf_status gpf_checkpoint_size(gpf_handle h, int64_t* bytes)
{
    gpf_status s = ckpt_ready(h);
    if (s) return s;
    if (!bytes) return fail(h, GPF_ERR_INVALID_ARGUMENT, "null output");
    *bytes = ckpt_bytes(h);
    return GPF_OK;
}
gpf_status gpf_checkpoint_save(gpf_handle h, void* out, int64_t bytes)
{
    gpf_status s = ckpt_ready(h);
    if (s) return s;
    if (!out || bytes != ckpt_bytes(h)) return fail(h, GPF_ERR_INVALID_ARGUMENT, "the buffer must hold exactly gpf_checkpoint_size bytes");
    // whatever is still deferred (lazy move, lazy search, un-gathered or un-scattered resample) becomes state first
    if ((s = check_ready(h)) || (s = finish_search(h)) || (s = materialize(h))) return s;
    CkptHeader hd{};
    hd.magic = CKPT_MAGIC; hd.version = 1; hd.model = h->cfg.model; hd.keep_prev = h->cfg.keep_prev; hd.W = h->W; hd.n_params = h->cfg.n_params;
    hd.has_prev = h->has_prev ? 1 : 0; hd.n_strata = h->args.n_strata; hd.interleaved = h->args.interleaved;
    hd.n = h->n; hd.n_global = h->cfg.n_global; hd.gid0 = h->cfg.gid0; hd.seed = h->cfg.seed; hd.epoch = h->epoch;
    hd.logK = h->args.logK;
    for (int i = 0; i < MAX_PARAMS; ++i) hd.params[i] = h->args.P[i];
    for (int i = 0; i < MAX_OBS; ++i) hd.obs[i] = h->args.obs[i];
    for (int i = 0; i < MAX_STRATA; ++i) hd.strata[i] = h->args.strata[i];
    for (int i = 0; i < 4; ++i) hd.q[i] = h->args.q[i];
    char* o = static_cast<char*>(out) + sizeof(CkptHeader);
    const size_t rb = (size_t)h->n * h->W * 8, wb = (size_t)h->n * 8, ab = (size_t)h->n * 4;
    HIP_TRY(h, hipMemcpyAsync(&hd.lml_est, reinterpret_cast<const char*>(h->sc.p) + offsetof(Scalars, lml_est), sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(o, h->rows[h->cur], rb, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(o + rb, h->lw, wb, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(o + rb + wb, h->anc, ab, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if ((s = check_scan_timeout(h))) return s;
    memcpy(out, &hd, sizeof(hd));
    return GPF_OK;
}
gpf_status gpf_checkpoint_load(gpf_handle h, const void* in, int64_t bytes)
{
    gpf_status s = ckpt_ready(h);
    if (s) return s;
    if (!in || bytes < (int64_t)sizeof(CkptHeader)) return fail(h, GPF_ERR_INVALID_ARGUMENT, "not a checkpoint");
    CkptHeader hd;
    memcpy(&hd, in, sizeof(hd));
    if (hd.magic != CKPT_MAGIC || hd.version != 1) return fail(h, GPF_ERR_INVALID_ARGUMENT, "not a checkpoint of this library version");
    bool same = hd.model == h->cfg.model && hd.keep_prev == h->cfg.keep_prev && hd.W == h->W && hd.n == h->n && hd.n_global == h->cfg.n_global &&
                hd.gid0 == h->cfg.gid0 && hd.seed == h->cfg.seed && hd.n_params == h->cfg.n_params;
    for (int i = 0; same && i < hd.n_params; ++i) same = memcmp(&hd.params[i], &h->args.P[i], sizeof(double)) == 0;
    if (!same) return fail(h, GPF_ERR_INVALID_ARGUMENT, "the checkpoint was taken of a filter with another gpf_config (model, parameters, particle counts, gid0, seed, keep_prev)");
    if (bytes != ckpt_bytes(h)) return fail(h, GPF_ERR_INVALID_ARGUMENT, "truncated checkpoint");
    if (h->hist_on) return fail(h, GPF_ERR_STATE, "a filter with a trajectory store cannot load a checkpoint (the store is not part of it)");
    if (gpf_status b = fwd_refused(h, "gpf_checkpoint_load")) return b;   // (the statistics are not part of a checkpoint either)
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    for (gpf_filter* v : h->blk_views) gpf_destroy(v);
    h->blk_views.clear();
    // the state is replaced: nothing deferred survives
    h->pending_move = false; h->pending_search = false; h->pending_gather = false; h->pending_fill = false;
    h->pending_packed = false; h->pend_ring = false;
    const char* o = static_cast<const char*>(in) + sizeof(CkptHeader);
    const size_t rb = (size_t)h->n * h->W * 8, wb = (size_t)h->n * 8, ab = (size_t)h->n * 4;
    HIP_TRY(h, hipMemcpyAsync(h->rows[h->cur], o, rb, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(h->lw, o + rb, wb, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(h->anc, o + rb + wb, ab, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(reinterpret_cast<char*>(h->sc.p) + offsetof(Scalars, lml_est), &hd.lml_est, sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->epoch = hd.epoch; h->has_prev = hd.has_prev != 0; h->initialized = true;
    h->args.n_strata = hd.n_strata; h->args.interleaved = hd.interleaved; h->args.logK = hd.logK;
    for (int i = 0; i < MAX_OBS; ++i) h->args.obs[i] = hd.obs[i];
    for (int i = 0; i < MAX_STRATA; ++i) h->args.strata[i] = hd.strata[i];
    for (int i = 0; i < 4; ++i) h->args.q[i] = hd.q[i];
    h->blk_obs_size = 0;
    h->residual_scanned = false; h->push_counted = false; h->gsum_ok = false; h->ch0_offsets = false;
    weights_written(h, false);
    return GPF_OK;
}

gpf_status gpf_history_mean(gpf_handle h, int32_t step, int32_t column, double* out) { return history_stat(h, step, column, out, false); }
gpf_status gpf_history_var(gpf_handle h, int32_t step, int32_t column, double* out) { return history_stat(h, step, column, out, true); }


} // extern "C"
