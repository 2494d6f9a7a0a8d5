// libgpf_store.hip -- the trajectory store's host side (the store itself is fed by hist_begin_step / hist_snapshot / hist_on_resample, libgpf_core.hip):
// enabling it, a past step's column / mean / variance / proportion along the ancestry, and the queries of the block-wise store -- past moments and
// proportions per block, sampled trajectories, backward simulation, marginal and pairwise smoothing, the most probable path.  The smoothers' and the
// path's kernels are instantiated in units of their own (libgpf_smooth / _pairs / _map .hip); the other four queries' kernels here, where they are the
// parent's instruction for instruction (tools/isa_diff.py).
// Buffers: the store's snapshots and device tables are members of the handle; an output's device copy is scratch of the one call (StoreOut).
#include "gpf_host.hpp"

using namespace gpf;
using namespace gpfh;

namespace gpfh {

namespace {

// column `column` of time step `step` (1-based, like the t of the Julia address t => :name) into h->dtmp
gpf_status history_values(gpf_handle h, int32_t step, int32_t column)
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
gpf_status history_stat(gpf_handle h, int32_t step, int32_t column, double* out, bool variance)
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

// The preamble of a query of the block-wise store, in ONE order ("the gate of the block-wise calls"): the gate, the query's own arguments,
// the step range (which brings the filter up to date), the 2^31 limits, the recorded block sizes, the device tables.  All but the tables change nothing.
// the gate of the queries; block_size comes back clamped.  needs_weights: the queries that read the store's weight records and evaluate the transition density
gpf_status block_store_gate(gpf_handle h, int64_t& block_size, const char* who, bool needs_weights = false)
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
gpf_status block_store_steps(gpf_handle h, int64_t block_size, int32_t step_lo, int32_t step_hi, const char* who, StoreSteps& r)
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
gpf_status block_store_draws(gpf_handle h, const StoreSteps& r, int32_t n_samples, const char* who, int64_t* draws)
{
    const int64_t lim = (int64_t)1 << 31, row = r.n_steps * h->d;
    *draws = r.nblocks * n_samples;
    if (*draws >= lim || row >= lim || *draws >= (lim + row - 1) / row)
        return fail(h, GPF_ERR_INVALID_ARGUMENT, std::string(who) + ": n_blocks * n_samples and n_blocks * n_samples * n_steps * dim must stay below 2^31");
    return GPF_OK;
}
// every walked step above step_lo reads the observation rows it was entered with, by the particle's block: a block-wise step of this block size
gpf_status block_store_sizes(gpf_handle h, int64_t block_size, int T, int32_t step_lo, const char* who)
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
gpf_status block_store_tables(gpf_handle h, bool with_weights)
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
void block_store_walk_args(gpf_handle h, const StoreSteps& r, int32_t step_lo, int32_t step_hi, int64_t block_size, StoreWalkArgs& a)
{
    a.maps = h->hist_dev_maps; a.hx = h->hist_dev_x; a.hlw = h->hist_dev_lw; a.hobs = h->hist_dev_obs; a.lw = h->lw;
    a.T = r.T; a.lo0 = step_lo - 1; a.hi0 = step_hi - 1;
    a.n = h->n; a.nb = block_size; a.nblocks = r.nblocks;
}
// One output of a query: `count` elements of device scratch of this call (up to 16 GB of trajectories are nothing to keep on a handle; freed on return --
// hipFree waits for the launch) and where the caller wants them.  Allocated only for an output that was asked for (host != nullptr), or `always`: scratch
// the kernel needs whatever was asked for.  Reads as its device pointer (nullptr: not wanted) and as the copy block_out makes of it
template <class T>
struct StoreOut {
    Dev<T> dev; T* host; size_t count;
    StoreOut(T* host_, size_t count_) : host(host_), count(count_) {}
    gpf_status alloc(gpf_handle h, bool always = false) { return host || always ? dev.alloc(h, count) : GPF_OK; }
    operator T*() const { return dev.p; }
    operator OutCopy() const { return OutCopy{dev.p, host, count * sizeof(T)}; }
};
// what both estimate queries do once the gate and their own arguments have passed: the current step is snapshotted and the maps of the steps
// T, T-1, ..., step+1 go to h->hist_dev_maps (as history_values): *n_maps of them
gpf_status block_hist_prepare(gpf_handle h, int32_t step, int* n_maps)
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
struct TrajLaunch { int T, lo0, hi0; int64_t nb, nblocks; int n_samples; double* traj; int64_t* idx; };
template <int D>
void launch_block_sample_traj(gpf_filter* h, const TrajLaunch& a)
{
    team_dispatch(a.nb, a.nblocks, [&](auto TEAM, auto ITEMS, dim3 grid) {
        GPF_LAUNCH((k_block_sample_traj<D, TEAM, ITEMS>), grid, dim3(BLOCK), 0, h->stream, h->hist_dev_maps.p, h->hist_dev_x.p, a.T, a.lo0, a.hi0, h->lw, h->n, a.nb, a.nblocks,
                   a.n_samples, h->cfg.seed, h->epoch, a.traj, a.idx);
    });
}
template <int M>
void launch_block_backward(gpf_filter* h, const BackArgs& a, const AncArgs& x)
{
    team_dispatch(a.nb, a.nblocks, [&](auto TEAM, auto ITEMS, dim3 grid) {
        // (the draws of a block are independent: with few blocks they are dealt to gridDim.y workgroups per block, so that the launch fills the chip)
        grid.y = (unsigned)std::max<int64_t>(1, std::min<int64_t>(a.n_samples, 2048 / std::max<int64_t>(1, (int64_t)grid.x)));
        GPF_LAUNCH((k_block_backward<M, TEAM, ITEMS>), grid, dim3(BLOCK), 0, h->stream, a, x);
    });
}

} // namespace
} // namespace gpfh

extern "C" {

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

gpf_status gpf_history_column(gpf_handle h, int32_t step, int32_t column, double* out, int64_t n)
{
    if (!h) return fail(nullptr, GPF_ERR_INVALID_ARGUMENT, "null handle");
    if (!out || n != h->n) return fail(h, GPF_ERR_INVALID_ARGUMENT, "bad output array");
    gpf_status s = history_values(h, step, column);
    if (s) return s;
    return copy_out(h, h->dtmp, out, (size_t)n * sizeof(double));
}
gpf_status gpf_history_mean(gpf_handle h, int32_t step, int32_t column, double* out) { return history_stat(h, step, column, out, false); }
gpf_status gpf_history_var(gpf_handle h, int32_t step, int32_t column, double* out) { return history_stat(h, step, column, out, true); }
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
    StoreOut<double> traj(traj_out, (size_t)draws * (size_t)r.n_steps * (size_t)h->d); StoreOut<int64_t> idx(idx_out, (size_t)draws);
    if ((s = block_store_tables(h, false)) || (s = traj.alloc(h)) || (s = idx.alloc(h))) return s;
    const TrajLaunch a{r.T, step_lo - 1, step_hi - 1, block_size, r.nblocks, (int)n_samples, traj, idx};
    DISPATCH_D(h, (launch_block_sample_traj<DD>(h, a)));
    HIP_TRY(h, hipGetLastError());
    if ((s = block_out(h, {traj, idx}))) return s;
    h->epoch += 1;                                                // as gpf_sample_unweighted: the draws' slots are not read again
    return GPF_OK;
}
// ---- backward simulation per block (gpf.h gpf_block_backward_sample): the step-T draw and the whole backward pass of all blocks and draws in one launch
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
    StoreOut<double> traj(traj_out, (size_t)draws * (size_t)r.n_steps * (size_t)h->d); StoreOut<int64_t> idx(idx_out, (size_t)draws * (size_t)r.n_steps);
    if ((s = block_store_tables(h, true)) || (s = traj.alloc(h)) || (s = idx.alloc(h))) return s;
    BackArgs a{};
    a.maps = h->hist_dev_maps; a.hx = h->hist_dev_x; a.hlw = h->hist_dev_lw; a.hobs = h->hist_dev_obs; a.lw = h->lw;
    a.T = r.T; a.lo0 = step_lo - 1; a.hi0 = step_hi - 1; a.n_samples = (int)n_samples;
    a.n = h->n; a.nb = block_size; a.nblocks = r.nblocks; a.seed = h->cfg.seed; a.epoch = h->epoch;
    a.traj = traj; a.idx = idx;
    const AncArgs x = anc_args(h);
    DISPATCH_MODEL(h, (launch_block_backward<MM>(h, a, x)));
    HIP_TRY(h, hipGetLastError());
    if ((s = block_out(h, {traj, idx}))) return s;
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
    StoreOut<double> mean(mean_out, (size_t)cells * (size_t)h->d), var(var_out, (size_t)cells * (size_t)h->d), w(weights_out, (size_t)cells * (size_t)block_size);
    StoreOut<int64_t> blocks(blocks_out, (size_t)cells);
    if ((s = block_store_tables(h, true)) || (s = mean.alloc(h)) || (s = var.alloc(h)) || (s = w.alloc(h)) || (s = blocks.alloc(h))) return s;
    SmoothArgs a{};
    block_store_walk_args(h, r, step_lo, step_hi, block_size, a);
    a.mean = mean; a.var = var;
    a.wout = w; a.blocks = blocks;
    launch_block_smooth(h, a, anc_args(h));
    HIP_TRY(h, hipGetLastError());
    // (nothing was drawn: the epoch stays)
    return block_out(h, {mean, var, w, blocks});
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
    StoreOut<double> mean(mean_out, (size_t)cells * (size_t)h->d), second(second_out, (size_t)cells * (size_t)dd),
                     cross(cross_out, (size_t)(r.nblocks * (r.n_steps - 1)) * (size_t)dd);
    StoreOut<int64_t> blocks(blocks_out, (size_t)cells);
    if ((s = block_store_tables(h, true)) || (s = mean.alloc(h)) || (s = second.alloc(h)) || (s = cross.alloc(h)) || (s = blocks.alloc(h))) return s;
    PairArgs a{};
    block_store_walk_args(h, r, step_lo, step_hi, block_size, a);
    a.mean = mean; a.second = second;
    a.cross = cross; a.blocks = blocks;
    launch_block_pairs(h, a, anc_args(h));
    HIP_TRY(h, hipGetLastError());
    // (nothing was drawn: the epoch stays)
    return block_out(h, {mean, second, cross, blocks});
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
    StoreOut<double> path(path_out, (size_t)cells * (size_t)h->d), logp(logp_out, (size_t)r.nblocks); StoreOut<int64_t> idx(idx_out, (size_t)cells);
    // the back-pointers (2 bytes per particle and step, rows padded to 16 bytes) and the lineage blocks: scratch of this call like the outputs' device
    // copies -- 198 MB at 10^4 blocks of 100 and T = 100 are nothing to keep on a handle -- that goes to no caller and is needed always
    const int64_t bsp = (block_size + 7) / 8 * 8;
    StoreOut<uint16_t> ptr(nullptr, (size_t)std::max(r.T - 1, 1) * (size_t)r.nblocks * (size_t)bsp); StoreOut<int32_t> lin(nullptr, (size_t)r.nblocks * (size_t)r.T);
    if ((s = block_store_tables(h, true)) || (s = path.alloc(h)) || (s = idx.alloc(h)) || (s = logp.alloc(h)) || (s = ptr.alloc(h, true)) || (s = lin.alloc(h, true))) return s;
    MapArgs a{};
    block_store_walk_args(h, r, step_lo, step_hi, block_size, a);
    a.path = path; a.idx = idx; a.logp = logp;
    a.ptr = ptr; a.lin = lin; a.bsp = bsp;
    launch_block_map(h, a, anc_args(h));
    HIP_TRY(h, hipGetLastError());
    // (nothing was drawn: the epoch stays)
    return block_out(h, {path, idx, logp});
}

} // extern "C"
