// libgpf_aux.hip -- what widened around the hot path and is neither block-wise (libgpf_blocks.hip) nor the trajectory store (libgpf_store.hip):
// weighted statistics (gpf_mean / gpf_var and the tree sum the store's statistics share), sub-state views (src/view.jl), the resize family with
// coalesce / introduce (src/resize.jl), checkpoint / resume.
// It also instantiates k_init / k_step / k_move of the block-wise calls (launch_init_blk / launch_step_blk / launch_move_blk, called from libgpf_blocks.hip):
// their code and k_introduce's depend on sharing a unit -- with the three in libgpf_blocks.hip, or the propagate alone left here, four k_introduce, four
// k_init and two k_move instantiations come out different (tools/isa_diff.py) -- and gpf_k_coalesce.hpp is included only here.
// Buffers: the scratch of one call is a local Dev<T> (gpf_host.hpp Owned).
#include "gpf_host.hpp"
#include "gpf_k_coalesce.hpp"

using namespace gpf;
using namespace gpfh;

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

// ---- the per-particle kernels of the block-wise calls (libgpf_blocks.hip), launched from there by run-time values
// block-wise initialise / propagate / move (ModelArgs::blk_*): no fused gather (a block resample gathers eagerly).  MODE 0: the default proposal;
// 2: stratified; 4 (propagate): per block the native proposal or the default one (ModelArgs::blk_prop).
// BP: per-block parameters are set (gpf_set_block_params) -- the kernels read block b's row of ModelArgs::blk_params instead of P
// MODE_REF: MODE 0 with slot 0 of every block pinned to its reference row (ModelArgs::blk_ref, conditional SMC)
template <int M, int MODE, bool BP>
static void launch_init_blk_as(gpf_filter* h, int grid)
{
    if constexpr (MODE == 2 && !Model<M>::HAS_STRATA) { (void)h; (void)grid; return; }
    else GPF_LAUNCH((k_init<M, MODE, true, BP>), dim3(grid), dim3(BLOCK), 0, h->stream, h->args, h->cfg.seed, h->epoch,
                    h->cfg.gid0, h->n, h->W, h->rows[h->cur], h->lw, next_slots(h));
}
template <int M, int MODE, bool KEEP, bool BP>
static void launch_step_blk_as(gpf_filter* h, int grid)
{
    constexpr int Wc = row_width(Model<M>::D, KEEP);
    if constexpr ((MODE == 2 && !Model<M>::HAS_STRATA) || (MODE == 4 && !Model<M>::HAS_PROPOSAL)) { (void)h; (void)grid; return; }
    else GPF_LAUNCH((k_step<M, Wc, KEEP, false, MODE, false, true, BP>), dim3(grid), dim3(BLOCK), 0, h->stream, h->args, h->cfg.seed, h->epoch,
                    h->cfg.gid0, h->n, h->anc, h->rows[h->cur], h->rows[1 - h->cur], h->lw, next_slots(h), PackedCommit{});
}
template <int M, bool RW, bool BP>
static void launch_move_blk_as(gpf_filter* h, int grid, int n_iters)
{
    constexpr int Wc = row_width(Model<M>::D, true);
    GPF_LAUNCH((k_move<M, Wc, RW, false, false, true, BP>), dim3(grid), dim3(BLOCK), 0, h->stream, h->args, h->cfg.seed, h->epoch,
                       h->cfg.gid0, h->n, (int)h->has_prev, n_iters, h->anc, h->rows[h->cur], h->rows[1 - h->cur], h->lw,
                       h->acc_part.p, RW ? next_slots(h) : MaxSlots{nullptr, nullptr});
}
// mode: 0 | 2 | MODE_REF, and 4 for the propagate; keep_prev and the per-block parameters are the handle's
void launch_init_blk(gpf_filter* h, int grid, int mode)
{
    bool_dispatch(h->bp_size > 0, [&](auto BP) {
        if (mode == MODE_REF) { DISPATCH_MODEL(h, (launch_init_blk_as<MM, MODE_REF, BP>(h, grid))); }
        else if (mode == 2)   { DISPATCH_MODEL(h, (launch_init_blk_as<MM, 2, BP>(h, grid))); }
        else                  { DISPATCH_MODEL(h, (launch_init_blk_as<MM, 0, BP>(h, grid))); }
    });
}
void launch_step_blk(gpf_filter* h, int grid, int mode)
{
    bool_dispatch(h->cfg.keep_prev != 0, h->bp_size > 0, [&](auto KEEP, auto BP) {
        if (mode == MODE_REF) { DISPATCH_MODEL(h, (launch_step_blk_as<MM, MODE_REF, KEEP, BP>(h, grid))); }
        else if (mode == 4)   { DISPATCH_MODEL(h, (launch_step_blk_as<MM, 4, KEEP, BP>(h, grid))); }
        else if (mode == 2)   { DISPATCH_MODEL(h, (launch_step_blk_as<MM, 2, KEEP, BP>(h, grid))); }
        else                  { DISPATCH_MODEL(h, (launch_step_blk_as<MM, 0, KEEP, BP>(h, grid))); }
    });
}
void launch_move_blk(gpf_filter* h, int grid, int n_iters, bool reweight)
{
    bool_dispatch(reweight, h->bp_size > 0, [&](auto RW, auto BP) { DISPATCH_MODEL(h, (launch_move_blk_as<MM, RW, BP>(h, grid, n_iters))); });
}

namespace {

gpf_status wstat(gpf_handle h, int32_t column, double* out, bool variance)
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

gpf_status view_create_impl(gpf_handle parent, int64_t start, int64_t step, int64_t count, const int64_t* index, gpf_handle* out)
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
gpf_status resize_ready(gpf_handle h, bool bump = true)
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
void set_count(gpf_filter* h, int64_t n_new)
{
    h->n = n_new; h->cfg.n_particles = n_new; h->cfg.n_global = n_new; h->cfg.gid0 = 0;
    if (h->blk_obs_size != 0) h->blk_obs_size = -1;              // per-block observations do not survive a change of the particle count
    h->blk_last = 0;
    // (forget(), not weights_written(): the resize family has never counted a mutation -- the views of a resized filter are stale by its generation)
    h->summary.forget();
    h->pending_gather = false; h->pending_fill = false; h->pending_packed = false; h->pending_search = false;
}

// pf_optimal_resize! (resize.jl:149-200): keep every particle with c w_i >= 1, resample the rest by systematic
// sampling, in exact fixed point.  n_new <= n_old.
gpf_status resize_optimal(gpf_handle h, int64_t n_new, int32_t check, int32_t* invalid)
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

// ---- pf_coalesce! / pf_introduce!: the launches (gpf_k_coalesce.hpp)
// device scratch of ONE call (hash table, slots, tile counts / the observation history) is a local Dev<T>: freed on every return path -- hipFree
// waits for the device, so no kernel of the call still reads it -- and never kept on the handle (46 MB at n = 10^6)
size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
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
void launch_coal_w(gpf_filter* h, const CoalArgs& a, int stage, double log_ratio = 0.0)
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

// ---- checkpoint / resume: everything a filter needs to continue bit for bit -- the population, its log-weights and parents, the log-ML
// estimate, the RNG epoch, the latest observation and strata -- as ONE host blob; loads into a handle created with the same gpf_config
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
} // namespace gpfh

extern "C" {

gpf_status gpf_mean(gpf_handle h, int32_t column, double* out) { return wstat(h, column, out, false); }
gpf_status gpf_var(gpf_handle h, int32_t column, double* out) { return wstat(h, column, out, true); }

// =================================================================================== sub-state views (src/view.jl)
gpf_status gpf_view_create(gpf_handle parent, int64_t start, int64_t count, gpf_handle* out)
{
    return gpf_view_create_strided(parent, start, 1, count, out);
}

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

gpf_status gpf_n_particles(gpf_handle h, int64_t* out)
{
    if (!h || !out) return fail(h, GPF_ERR_INVALID_ARGUMENT, "null argument");
    *out = h->n;
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

// =================================================================================== checkpoint / resume
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

} // extern "C"
