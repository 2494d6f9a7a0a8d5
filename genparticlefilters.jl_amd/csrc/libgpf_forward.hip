// libgpf_forward.hip -- forward-only smoothing per block (gpf_k_block_forward.hpp; gpf.h gpf_forward_enable_blocks / gpf_block_forward_moments): the
// kernels' instantiations, the mode's one generation of records, the two hooks of the block-wise calls (hist_begin_step, hist_on_resample in
// libgpf_core.hip) and the two entry points.  A translation unit of its own, for the reason libgpf_smooth.hip and libgpf_pairs.hip are:
// every other unit's device code stays what it was (tools/isa_diff.py; profiles/block_forward.md).
#include "gpf_host.hpp"

using namespace gpf;
using namespace gpfh;

namespace gpfh {

void fwd_free(gpf_filter* h)
{
    h->fwd_x.reset(); h->fwd_lw.reset();
    for (int k = 0; k < 2; ++k) { h->fwd_T[k].reset(); h->fwd_map[k].reset(); }
    h->fwd_steps = 0; h->fwd_map_set = false;
}
// the records of a filter of n particles: the previous step's columns and log-weights, the two halves of the statistics, the two maps
static gpf_status fwd_buffers(gpf_filter* h)
{
    const size_t n = (size_t)h->n, F = (size_t)fwd_F(h->d);
    if (h->fwd_lw.count == n) return GPF_OK;
    if (h->fwd_x) { HIP_TRY(h, hipStreamSynchronize(h->stream)); fwd_free(h); }   // (another particle count, or an allocation that failed half-way)
    gpf_status s;
    if ((s = h->fwd_x.alloc(h, n * (size_t)h->d))) return s;
    for (int k = 0; k < 2; ++k)
        if ((s = h->fwd_T[k].alloc(h, n * F)) || (s = h->fwd_map[k].alloc(h, n))) return s;
    return h->fwd_lw.alloc(h, n);                                 // (last: its count says the records are complete)
}
template <int M>
static void launch_block_forward_model(gpf_filter* h, const ForwardArgs& a, const AncArgs& x)
{
    const int64_t waves = a.nblocks * a.wpb;
    GPF_LAUNCH((k_block_forward<M>), dim3((unsigned)((waves + NWAVES - 1) / NWAVES)), dim3(BLOCK), 0, h->stream, a, x,
               (const double*)h->fwd_x.p, (const double*)h->fwd_lw.p, (const double*)h->fwd_T[h->fwd_cur].p, h->fwd_T[1 - h->fwd_cur].p);
}
// the statistics of the CURRENT step from the record of the previous one, as a close forms them (the filter is materialised: the callers see to it)
gpf_status fwd_form(gpf_filter* h)
{
    const int64_t bs = h->fwd_bsize;
    ForwardArgs a{};
    a.rows = h->rows[h->cur]; a.W = h->W; a.map = h->fwd_map_set ? h->fwd_map[h->fwd_map_cur] : nullptr; a.obs = h->blk_obs;
    a.n = h->n; a.nb = bs; a.nblocks = (h->n + bs - 1) / bs; a.wpb = (int)((bs + WAVE - 1) / WAVE); a.first = h->fwd_steps == 1 ? 1 : 0;
    const AncArgs x = anc_args(h);                                // (the parameters current now: the filter's, or every block's own row)
    DISPATCH_MODEL(h, (launch_block_forward_model<MM>(h, a, x)));
    HIP_TRY(h, hipGetLastError());
    return GPF_OK;
}
gpf_status fwd_begin_step(gpf_filter* h, bool first)
{
    if (first) {
        if (h->fwd_bsize < 1) return fail(h, GPF_ERR_STATE, "forward smoothing per block follows the block-wise calls: begin with gpf_initialize_blocks");
        if (h->d != 1 && h->d != 2 && h->d != 4) return fail(h, GPF_ERR_STATE, "latent dimension");
        gpf_status s = fwd_buffers(h);
        if (s) return s;
        h->fwd_steps = 1; h->fwd_cur = 0; h->fwd_map_set = false;
        return GPF_OK;
    }
    if (h->fwd_steps < 1) return fail(h, GPF_ERR_STATE, "forward smoothing per block: nothing is initialised");
    // ---- the close of the step that ends: its statistics, then its columns and log-weights, in its final order
    gpf_status s = fwd_form(h);
    if (s) return s;
    GPF_LAUNCH(k_hist_snapshot, dim3(grid_for(h, h->n * h->d, 8)), dim3(BLOCK), 0, h->stream, h->rows[h->cur], h->W, h->d, h->n, h->fwd_x.p);
    GPF_LAUNCH(k_hist_record, dim3(grid_for(h, h->n, 8)), dim3(BLOCK), 0, h->stream, (const double*)h->lw, h->n, (const double*)nullptr, (int64_t)0, h->fwd_lw.p, (double*)nullptr);
    HIP_TRY(h, hipGetLastError());
    h->fwd_cur ^= 1; h->fwd_steps += 1; h->fwd_map_set = false;
    return GPF_OK;
}
// (two maps used in turn: nothing is allocated, synchronised or freed here -- the kernels of one stream run in order)
gpf_status fwd_on_resample(gpf_filter* h, int64_t block_size)
{
    if (h->fwd_steps < 1) return GPF_OK;
    const int32_t* old = h->fwd_map_set ? h->fwd_map[h->fwd_map_cur] : nullptr;
    int32_t* neu = h->fwd_map[1 - h->fwd_map_cur];
    if (block_size > 0) GPF_LAUNCH(k_hist_compose_blocks, dim3(grid_for(h, h->n, 8)), dim3(BLOCK), 0, h->stream, (const int32_t*)h->anc, (const int32_t*)h->blk_mask.p, block_size, old, h->n, neu);
    else GPF_LAUNCH(k_hist_compose, dim3(grid_for(h, h->n, 8)), dim3(BLOCK), 0, h->stream, (const int32_t*)h->anc, old, h->n, neu);
    HIP_TRY(h, hipGetLastError());
    h->fwd_map_cur ^= 1; h->fwd_map_set = true;
    return GPF_OK;
}
template <int D>
static void launch_block_forward_reduce_d(gpf_filter* h, const double* T, double* out)
{
    const int64_t bs = h->fwd_bsize, nblocks = (h->n + bs - 1) / bs;
    team_dispatch(bs, nblocks, [&](auto TEAM, auto ITEMS, dim3 grid) {
        GPF_LAUNCH((k_block_forward_reduce<D, TEAM, ITEMS>), grid, dim3(BLOCK), 0, h->stream, T, (const double*)h->rows[h->cur], h->W, (const double*)h->lw, h->n, bs, nblocks, out);
    });
}
void launch_block_forward_reduce(gpf_filter* h, const double* T, double* out)
{
    DISPATCH_D(h, (launch_block_forward_reduce_d<DD>(h, T, out)));
}

} // namespace gpfh

extern "C" {

// ---- the entry points (gpf.h): the additive smoothing functionals of particle EM after every step, from the one generation of records above
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

} // extern "C"
