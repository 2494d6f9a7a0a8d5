// K11g: a conditional SMC sweep per block in one launch, the path drawn by the ancestral walk or by backward simulation  (part of gpf_kernels.hpp; include that header, not this file)
#pragma once

namespace gpf {
// ----------------------------------------------------------------------------- the conditional filter of many small filters, block by block
// gpf_sweep_blocks (gpf.h): one sweep of particle Gibbs (Andrieu, Doucet & Holenstein 2010), with ancestor sampling (Lindsten, Jordan &
// Schoen 2014) where AS,
//     for t in 1:T;  pf_resample_blocks(state, bs, conditional = true[, reference = ref[:, t], observations = ys[:, t]], ess_frac, check = false)
//                    pf_update_blocks(state, ..., ys[:, t], bs, reference = ref[:, t]);  end
//     path = block_sample_trajectories(state, bs, 1)
// in ONE launch and without a trajectory store.  Team b (team_dispatch) runs all n_steps iterations of block b as k_block_run does, then draws the
// block's one path and walks it back.  Per step, statement for statement:
//   gate       the weight summary the previous step closed with (run_summary), as in k_block_run;
//   ancestor   AS, blocks that resample: k_block_resample_anc's pass -- lwa_i = lw_i + logtrans(P_b, x_i, ref[b][t], ys[b][t]), maximum and flags,
//              exp_fix, scan, the CDF in s_cdf, the team-uniform search for a_0 under slot 0's own counter of epoch E + 2t; invalid or all -Inf ancestor
//              weights: a_0 = 0.  Without AS a_0 = 0 (k_block_resample<METHOD_COND>).  Then the weight CDF overwrites s_cdf;
//   slots      the ancestor by lds_upper_bound, slot 0 takes a_0; its row goes from slab t straight into Model<M>::sample in registers under epoch
//              E + 2t + 1, TAG_UPDATE; every lane draws, then slot 0's latent is overwritten by ref[b][t] and its increment is loglik of that row
//              (MODE_REF of k_step); lw = (new weight | lw) + ll;
//   close      run_sync, run_summary: step t's outputs and step t + 1's gate.
// The genealogy slabs ARE the row buffers: slabs = [n_steps + 1][n][W] rows, par = [n_steps][n] 16-bit block-local parents, scratch of the call.  Step t
// reads its ancestors' rows in slab t and writes the propagated rows into slab t + 1; a block that does not resample reads its own rows in slab t and
// writes slab t + 1 as well.  Nothing flips, nothing is propagated in place, and the record of a step is the store the step makes anyway.  Slab 0 is the
// handle's rows on entry (the team copies its block in), the last slab goes back into the handle's buffer behind the last step.  A step in which the
// block did not resample writes no parent words: the walk reads the step's resample word (team-uniform) and stays where it is.
// The draw: after the last step the summary's q, scanned, is the CDF k_block_sample_traj forms of the same weights (1 per particle for an all -Inf
// block); lane 0 of the team draws under slot b of epoch E + 2 n_steps, walks the 16-bit parents down the slabs and writes the block's
// [n_steps + 1][D] run of `path` from the last step down.  NaN / +Inf weights: index 0, NaN path.
// LDS: s_cdf and the reduction cells (16.2 kB in the workgroup shape).  Synchronisation: run_sync, as argued in gpf_k_block_run.hpp; no spin waits,
// nothing between workgroups; every loop is bounded by n_steps, cnt or log2 cnt.
//
// One kernel template serves both draws: BACK = false is all of the above; the forward part is written
// once and the two tails stand in the two branches of one `if constexpr` (profiles/block_series_kernels.md).
// ----------------------------------------------------------------------------- particle Gibbs with backward simulation, block by block
// BACK -- gpf_sweep_blocks_backward (gpf.h): the forward part above, then the path drawn by backward simulation (Whiteley 2010; Lindsten &
// Schoen 2013) instead of the ancestral walk -- bit for bit
//     for t in 1:T;  pf_resample_blocks(state, bs, conditional = true[, reference = ref[:, t], observations = ys[:, t]], ess_frac, check = false)
//                    pf_update_blocks(state, ..., ys[:, t], bs, reference = ref[:, t]);  end
//     path, indices = block_backward_trajectories(state, bs, 1, return_indices = true)
// on a filter with a store that records weights, in ONE launch and without that store.
// What the store of the loop holds, in terms of the sweep: the store closes a step when the NEXT update begins, so step s < T is recorded in its FINAL
// order -- behind the resample of iteration s (0-based) -- and step T as it stands.  With X_s = row slab s, go_s / par_s the resample word and the
// 16-bit parents of iteration s, and r_s(j) = go_s ? par_s[j] : j (r_T = the identity):
//     hist_x[s][j] = X_s[r_s(j)],    hist_lw[s][j] = the weight slot j enters iteration s's propagate with (the new weight | its own),
//     maps[s][j] = r_s(j),           hist_obs[s] = the block's series at iteration s - 1.
// Forward part: the steps above plus ONE store per particle and step: the
// weight lw_in the slot loop adds the increment to also goes into slab t of lws = [n_steps][n].  Step T's weights are the handle's.
// Backward part: k_block_backward's statements with n_samples = 1, on those slabs, by the WHOLE team per step (the ancestral walk was lane 0's chain
// of dependent 16-bit loads; this pass is cnt transition densities, a maximum, a scan and a search per step, ITEMS consecutive candidates per lane):
//   step T     the q the last run_summary left in registers, scanned into s_cdf, is the weight CDF; p = upper_bound(cdf, mulhi64(U, S)),
//              U = resample_u64(seed, b, E + 2 n_steps) -- slot b, as draw 0 of block b among the store's draws;
//   step s     n_steps .. 1, p the held particle in step s's final order: pm = r_s(p) its recorded parent, which is also its row in slab s -- x_held =
//              X_s[pm], one broadcast address; ob = the series at iteration s - 1, zero-padded; candidates i of step s - 1's final order, their rows
//              gathered through par_{s-1}: lwa_i = lws[s - 1][i] + logtrans(P_b, X_{s-1}[r_{s-1}(i)], x_held, ob) (anc_weights' statements with the
//              gather in the address); team_max_flags, exp_fix(lwa - m', K), scan into s_cdf, sync,
//              new p = upper_bound(cdf, mulhi64(U_s, S')) with U_s = resample_u64(seed, b, E + 2 n_steps + (n_steps - s + 1)), sync;
//   fallback   flags of lwa hold NaN, +Inf or ALL_NEGINF -> new p = pm: a 16-bit load where the block resampled in iteration s, the same particle else;
//   bad block  final weights with NaN / +Inf: indices 0 and NaN paths.
// The lineage never leaves its block (no resample across blocks inside the sweep), so k_block_backward's map / division / foreign-block arithmetic is
// gone and K, cnt and P_b are the block's own.  Lane 0 writes the path row and the 1-based global index (final order) of every step.
// Synchronisation: the last forward step's run_sync orders every row, weight, parent and resample word of the slabs before the first backward load;
// the backward part writes only outputs.  The two team_syncs around every search of s_cdf are k_block_backward's.  LDS is the plain sweep's.  No spin
// waits, nothing between workgroups; every loop is bounded by n_steps, cnt or log2 cnt.
struct SweepArgs {
    double* rows;                                  // [n][W] the handle's current buffer: read on entry, holds the last slab on exit
    double* slabs;                                 // [n_steps + 1][n][W]
    uint16_t* par;                                 // [n_steps][n] parents, local to the block, of the steps in which the block resampled
    double* lw;                                    // [n]
    int32_t* anc;                                  // [n] the handle's parents (last write wins)
    int64_t n, nb, nblocks, gid0;
    uint64_t seed; uint32_t epoch;                 // E: the resample of step t runs under E + 2t, the propagate under E + 2t + 1, the draw under E + 2 n_steps
    int32_t n_steps;
    double ess_frac;                               // < 0: every block resamples at every step
    const double* P;                               // [MAX_PARAMS] the filter's parameters (device)
    const double* blk_params;                      // [nblocks][MAX_PARAMS] or null
    const double* obs; int64_t obs_blocks;         // [obs_blocks][n_steps][n_obs], the caller's layout; obs_blocks = nblocks | 1
    int32_t n_obs;
    const double* ref;                             // [nblocks][n_steps][D], the caller's layout
    const double* lml_est;
    double* ess_out; double* lml_out;              // [n_steps][nblocks]
    int32_t* res_out;                              // [n_steps][nblocks] the word of step t's resample (also what the walk reads)
    int32_t* flags_out;                            // [nblocks]
    double* blk_obs;                               // [nblocks][MAX_OBS] the last step's
    double* path;                                  // [nblocks][n_steps + 1][D]
    int64_t* idx_out;                              // [nblocks] 1-based index, inside the block, of the drawn final particle; BACK: [nblocks][n_steps + 1],
                                                   // 1-based GLOBAL indices in each step's final order
    double* lws;                                   // BACK: [n_steps][n] the log-weight slabs: what slot j enters iteration t's propagate with
};
template <int M, int W, bool AS, int TEAM, int ITEMS, bool BACK>    // W = row_width(Model<M>::D, false); BACK: the path by backward simulation
__global__ __launch_bounds__(BLOCK) void k_block_sweep(SweepArgs a)
{
    using Mo = Model<M>;
    constexpr int D = Mo::D;
    constexpr int TEAMS = BLOCK / TEAM, CAP = TEAM * ITEMS;        // blocks per workgroup, particles a team holds
    static_assert(TEAM == WAVE || TEAM == BLOCK, "a wave or the workgroup");
    static_assert(W >= D && W % 2 == 0, "rows are moved as 16-byte column pairs");
    static_assert(D == 1 || D % 2 == 0, "the path is written as words or 16-byte pairs");
    static_assert(BLK_MAX <= 65536, "16-bit parents");
    __shared__ uint64_t s_cdf_[BLOCK * ITEMS];                     // first the ancestor weights' CDF (AS), then the weights'; at the end the draw's (BACK: and every backward step's)
    __shared__ uint64_t s_x[NWAVES][4];
    __shared__ double s_m[NWAVES];
    __shared__ int s_f[NWAVES];
    const int tm = (int)threadIdx.x / TEAM, tl = (int)threadIdx.x % TEAM;
    const int64_t blk = (int64_t)blockIdx.x * TEAMS + tm;
    if (TEAM != BLOCK && blk >= a.nblocks) return;                 // (an idle wave: the wave-team path has no workgroup barrier)
    uint64_t* const s_cdf = s_cdf_ + tm * CAP;
    const int64_t b0 = blk * a.nb;
    const int cnt = (int)(a.n - b0 < a.nb ? a.n - b0 : a.nb);      // particles of this block
    const int K = fix_K(cnt);
    const double* const P = a.blk_params ? a.blk_params + blk * MAX_PARAMS : a.P;      // (team-uniform)
    const double* const obs_b = a.obs + (a.obs_blocks == 1 ? 0 : (size_t)blk * (size_t)a.n_steps * (size_t)a.n_obs);      // the block's series
    const double* const ref_b = a.ref + (size_t)blk * (size_t)a.n_steps * D;                                              // ... and retained path
    const double lml0 = *a.lml_est;
    double* const lw = a.lw + b0;
    const size_t slab = (size_t)a.n * W;                           // doubles per slab
    // ---- slab 0: the block's rows on entry
    for (int e = tl; e < cnt * (W / 2); e += TEAM)
        reinterpret_cast<double2*>(a.slabs + b0 * W)[e] = reinterpret_cast<const double2*>(a.rows + b0 * W)[e];
    run_sync<TEAM>();
    int flags_all = 0;
    double m; int f; uint64_t q[ITEMS]; uint64_t S_w; double ess;
    run_summary<TEAM, ITEMS>(lw, cnt, K, tl, s_m, s_f, s_x, m, f, q, S_w, ess);
#pragma unroll 1
    for (int t = 0; t < a.n_steps; ++t) {
        // ================ the conditional resample, epoch E + 2t
        const uint32_t ep_r = a.epoch + 2u * (uint32_t)t, ep_u = ep_r + 1u;
        const bool gate = a.ess_frac >= 0.0 ? (f == 0 && ess < a.ess_frac * (double)cnt) : true;
        const bool skip = (f & (FLAG_NAN | FLAG_POSINF)) != 0;     // NaN / +Inf: left as it stands (check = false)
        const bool go = gate && !skip;
        if (tl == 0) a.res_out[(int64_t)t * a.nblocks + blk] = (go ? 1 : 0) | ((gate ? f : 0) << 8);
        flags_all |= gate ? f : 0;
        double ob[MAX_OBS], xr[D];                                 // (team-uniform: the block's rows of step t)
        {
            const double* const orow = obs_b + (size_t)t * (size_t)a.n_obs;
#pragma unroll
            for (int k = 0; k < MAX_OBS; ++k) ob[k] = k < a.n_obs ? orow[k] : 0.0;
            const double* const rrow = ref_b + (size_t)t * D;
#pragma unroll
            for (int k = 0; k < D; ++k) xr[k] = rrow[k];
        }
        const double* const rows_in = a.slabs + (size_t)t * slab + b0 * W;
        double* const rows_out = a.slabs + ((size_t)t + 1) * slab + b0 * W;
        double* lws_t = nullptr;
        if constexpr (BACK) lws_t = a.lws + (size_t)t * (size_t)a.n + b0;
        uint16_t* const par = a.par + (size_t)t * (size_t)a.n + b0;
        uint64_t S = 0;
        int a0 = 0;                                                // slot 0's ancestor: itself, unless one is sampled
        if (go) {
            if (AS) {
                // ---- k_block_resample_anc: the ancestor weights, their maximum, flags and CDF; the team-uniform search
                double lwv[ITEMS], lwa[ITEMS];
#pragma unroll
                for (int k = 0; k < ITEMS; ++k) { const int i = ITEMS * tl + k; lwv[k] = i < cnt ? lw[i] : -__builtin_huge_val(); }
                anc_weights<M, W, ITEMS>(P, rows_in, cnt, tl, xr, ob, lwv, lwa);
                double m_a; int f_a;
                team_max_flags<TEAM, ITEMS>(lwa, tl, cnt, s_m, s_f, m_a, f_a);
                uint64_t qa[ITEMS];
#pragma unroll
                for (int k = 0; k < ITEMS; ++k) qa[k] = ITEMS * tl + k < cnt ? exp_fix(lwa[k] - m_a, K) : 0ull;
                const uint64_t S_a = team_scan_incl<TEAM, ITEMS>(qa, s_x);
#pragma unroll
                for (int k = 0; k < ITEMS; ++k) s_cdf[ITEMS * tl + k] = qa[k];
                team_sync<TEAM>();
                if (f_a == 0) a0 = lds_upper_bound(s_cdf, cnt, mulhi64(resample_u64(a.seed, (uint32_t)(a.gid0 + b0), ep_r), S_a));
                team_sync<TEAM>();                                 // (s_cdf is overwritten next)
            }
            S = team_scan_incl<TEAM, ITEMS>(q, s_x);
#pragma unroll
            for (int k = 0; k < ITEMS; ++k) s_cdf[ITEMS * tl + k] = q[k];
            team_sync<TEAM>();
        }
        const double new_lw = go ? lse_from(m, S, K, f) - log_((double)cnt) : 0.0;
        // ================ the slots: ancestor, then k_step's MODE_REF body under epoch E + 2t + 1
        for (int j = tl; j < cnt; j += TEAM) {                     // consecutive lanes, consecutive slots: coalesced stores
            const uint32_t slot = (uint32_t)(a.gid0 + b0 + j);
            int anc = j;
            if (go) {
                anc = lds_upper_bound(s_cdf, cnt, mulhi64(resample_u64(a.seed, slot, ep_r), S));
                if (j == 0) anc = a0;                              // the retained path
                a.anc[b0 + j] = anc;
                par[j] = (uint16_t)anc;
            }
            double r[W];
            {
                const double2* src = reinterpret_cast<const double2*>(rows_in + (size_t)anc * W);
#pragma unroll
                for (int c = 0; c < (D + 1) / 2; ++c) { const double2 v = src[c]; r[2 * c] = v.x; r[2 * c + 1] = v.y; }
            }
            const double lw_in = go ? new_lw : lw[j];
            if constexpr (BACK) lws_t[j] = lw_in;                  // (the store's record of step t in its final order)
            double xn[MAX_DIM];
            Mo::sample(P, false, r, ob, a.seed, slot, 0, ep_u, TAG_UPDATE, xn);
#pragma unroll
            for (int k = 0; k < D; ++k) xn[k] = j == 0 ? xr[k] : xn[k];      // (every lane draws; the pinned lane overwrites its draw)
            const double ll = Mo::loglik(P, xn, ob);
            double o[W];
#pragma unroll
            for (int k = 0; k < W; ++k) o[k] = 0.0;
#pragma unroll
            for (int k = 0; k < D; ++k) o[k] = xn[k];
            double2* dst = reinterpret_cast<double2*>(rows_out + (size_t)j * W);
#pragma unroll
            for (int c = 0; c < W / 2; ++c) dst[c] = make_double2(o[2 * c], o[2 * c + 1]);
            lw[j] = lw_in + ll;
        }
        run_sync<TEAM>();                                          // rows, weights and parents of this step: visible to the team (and s_cdf free again)
        // ================ k_block_stats: step t's outputs, step t + 1's gate and weights
        run_summary<TEAM, ITEMS>(lw, cnt, K, tl, s_m, s_f, s_x, m, f, q, S_w, ess);
        if (tl == 0) {
            a.ess_out[(int64_t)t * a.nblocks + blk] = f ? __builtin_nan("") : ess;
            a.lml_out[(int64_t)t * a.nblocks + blk] = (lml0 + lse_from(m, S_w, K, f)) - log_((double)cnt);
        }
    }
    if (tl == 0) a.flags_out[blk] = flags_all << 8;
    if (tl < MAX_OBS)                                              // the block's row of the handle's per-block observations: the last step's
        a.blk_obs[blk * MAX_OBS + tl] = tl < a.n_obs ? obs_b[(size_t)(a.n_steps - 1) * (size_t)a.n_obs + tl] : 0.0;
    // ---- the last slab into the handle's buffer (the last step's run_sync ordered the rows)
    {
        const double* const last = a.slabs + (size_t)a.n_steps * slab + b0 * W;
        for (int e = tl; e < cnt * (W / 2); e += TEAM)
            reinterpret_cast<double2*>(a.rows + b0 * W)[e] = reinterpret_cast<const double2*>(last)[e];
    }
    if constexpr (!BACK) {
        // ================ k_block_sample_traj with n_samples = 1: the draw from the final weights, the walk down the slabs
        const uint64_t S_d = team_scan_incl<TEAM, ITEMS>(q, s_x);
#pragma unroll
        for (int k = 0; k < ITEMS; ++k) s_cdf[ITEMS * tl + k] = q[k];
        team_sync<TEAM>();
        if (tl != 0) return;
        const bool bad = (f & (FLAG_NAN | FLAG_POSINF)) != 0;
        int p = -1;
        if (!bad) p = lds_upper_bound(s_cdf, cnt, mulhi64(resample_u64(a.seed, (uint32_t)blk, a.epoch + 2u * (uint32_t)a.n_steps), S_d));
        a.idx_out[blk] = (int64_t)p + 1;
        double* const out = a.path + (size_t)blk * ((size_t)a.n_steps + 1) * D;
        if (bad) {
            for (int e = 0; e < (a.n_steps + 1) * D; ++e) out[e] = __builtin_nan("");
            return;
        }
        for (int s = a.n_steps; s >= 0; --s) {
            const double* const x = a.slabs + (size_t)s * slab + (size_t)(b0 + p) * W;
            double* const o = out + (size_t)s * D;
            if constexpr (D == 1) o[0] = x[0];
            else {
#pragma unroll
                for (int c = 0; c < D / 2; ++c) reinterpret_cast<double2*>(o)[c] = reinterpret_cast<const double2*>(x)[c];
            }
            if (s > 0 && (a.res_out[(int64_t)(s - 1) * a.nblocks + blk] & 1)) p = (int)a.par[(size_t)(s - 1) * (size_t)a.n + b0 + p];
        }
    } else {
        // ================ k_block_backward with n_samples = 1: the draw from the final weights, then the whole team per step down the slabs
        double* const out = a.path + (size_t)blk * ((size_t)a.n_steps + 1) * D;
        int64_t* const iout = a.idx_out + (size_t)blk * ((size_t)a.n_steps + 1);
        if ((f & (FLAG_NAN | FLAG_POSINF)) != 0) {                     // (team-uniform)
            for (int e = tl; e < (a.n_steps + 1) * D; e += TEAM) out[e] = __builtin_nan("");
            for (int e = tl; e <= a.n_steps; e += TEAM) iout[e] = 0;
            return;
        }
        const uint32_t ep_d = a.epoch + 2u * (uint32_t)a.n_steps;
        const uint64_t S_d = team_scan_incl<TEAM, ITEMS>(q, s_x);
#pragma unroll
        for (int k = 0; k < ITEMS; ++k) s_cdf[ITEMS * tl + k] = q[k];
        team_sync<TEAM>();
        int p = lds_upper_bound(s_cdf, cnt, mulhi64(resample_u64(a.seed, (uint32_t)blk, ep_d), S_d));      // (team-uniform, local to the block)
        team_sync<TEAM>();                                             // (s_cdf is overwritten next)
        int go_s = 0;                                                  // (step n_steps stands as the last propagate left it: r = the identity)
#pragma unroll 1
        for (int s = a.n_steps; ; --s) {
            // the recorded parent of the held particle -- a 16-bit load where the block resampled in iteration s -- is its row in slab s
            const int pm = go_s ? (int)a.par[(size_t)s * (size_t)a.n + b0 + p] : p;
            const double* __restrict__ xh = a.slabs + (size_t)s * slab + (size_t)(b0 + pm) * W;    // one broadcast address
            if (tl == 0) {
                double* const o = out + (size_t)s * D;
                if constexpr (D == 1) o[0] = xh[0];
                else {
#pragma unroll
                    for (int c = 0; c < D / 2; ++c) reinterpret_cast<double2*>(o)[c] = reinterpret_cast<const double2*>(xh)[c];
                }
                iout[s] = b0 + p + 1;
            }
            if (s == 0) break;
            go_s = a.res_out[(int64_t)(s - 1) * a.nblocks + blk] & 1;  // (team-uniform) iteration s - 1: the order of the candidates
            double xr[D], ob[MAX_OBS];
            load_latent<D>(xh, xr);
            {
                const double* const orow = obs_b + (size_t)(s - 1) * (size_t)a.n_obs;
#pragma unroll
                for (int k = 0; k < MAX_OBS; ++k) ob[k] = k < a.n_obs ? orow[k] : 0.0;
            }
            const double* __restrict__ plw = a.lws + (size_t)(s - 1) * (size_t)a.n + b0;
            const uint16_t* __restrict__ par = a.par + (size_t)(s - 1) * (size_t)a.n + b0;
            const double* __restrict__ rows_c = a.slabs + (size_t)(s - 1) * slab + b0 * W;
            double lwa[ITEMS];
#pragma unroll
            for (int k = 0; k < ITEMS; ++k) {                          // anc_weights, the candidate's row gathered through its parent
                const int i = ITEMS * tl + k;
                lwa[k] = -__builtin_huge_val();
                if (i < cnt) {
                    const int ci = go_s ? (int)par[i] : i;
                    double xp[D];
                    load_latent<D>(rows_c + (size_t)ci * W, xp);
                    lwa[k] = plw[i] + Mo::logtrans(P, xp, xr, ob);
                }
            }
            double m_a; int f_a;
            team_max_flags<TEAM, ITEMS>(lwa, tl, cnt, s_m, s_f, m_a, f_a);
            uint64_t qa[ITEMS];
#pragma unroll
            for (int k = 0; k < ITEMS; ++k) qa[k] = ITEMS * tl + k < cnt ? exp_fix(lwa[k] - m_a, K) : 0ull;
            const uint64_t S_a = team_scan_incl<TEAM, ITEMS>(qa, s_x);
#pragma unroll
            for (int k = 0; k < ITEMS; ++k) s_cdf[ITEMS * tl + k] = qa[k];
            team_sync<TEAM>();
            // every lane evaluates the draw (a team-uniform search of LDS); invalid ancestor weights: the recorded parent
            p = pm;
            if (f_a == 0) p = lds_upper_bound(s_cdf, cnt, mulhi64(resample_u64(a.seed, (uint32_t)blk, ep_d + (uint32_t)(a.n_steps - s + 1)), S_a));
            team_sync<TEAM>();                                         // (s_cdf is overwritten by the next step)
        }
    }
}

} // namespace gpf
