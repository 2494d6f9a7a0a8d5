// K11h: a whole series per block in one launch, with the rejuvenation moves inside  (part of gpf_kernels.hpp; include that header, not this file)
#pragma once

namespace gpf {
// ----------------------------------------------------------------------------- the full README loop of many small filters, block by block
// gpf_run_blocks_rejuvenate (gpf.h): the loop of README.md:60-79 per block on a keep_prev filter,
//     for t in 1:T
//         pf_resample_blocks(state, bs, method, ess_frac, check = false)                           epoch E + 3t
//         pf_rejuvenate_blocks(state, n_iters; method = move | reweight, only_resampled = true)    epoch E + 3t + 1
//         pf_update_blocks(state, ..., ys[:, t], bs)                                                epoch E + 3t + 2
//     end
// in ONE launch, one team per block as in k_block_run (gpf_k_block_run.hpp), whose gate, order, CDFs, search, summary and barrier (run_summary,
// run_sync) these are, statement for statement.  What is this kernel's own is the slot body and what moves around it:
//   one load, one store    the slot loads its ancestor's FULL row [x | x_{t-1}] as 16-byte pairs, runs the n_iters iterations of k_move's selection
//                          variant (PROP = false; gpf_k_step.hpp) on x in registers against x_{t-1} and the block's PREVIOUS observation, draws x_new
//                          from the moved x (k_step's default proposal) and stores [x_new | moved x] once.  The loop stores and reloads that row
//                          three times per step.  A block that does not resample skips the move team-uniformly (iters = 0) and propagates in place;
//                          the only lane divergence of the move is the MH accept, and that is a select;
//   the previous observation  obp: the handle's per-block row, read once before the loop; then step t's zero-padded row becomes step t + 1's obp in
//                          registers.  The handle's row is written once after the loop, as k_block_run writes it;
//   move-reweight weights  (new_lw + wsum) + ll is formed in registers -- rejuvenate.jl:86's sum, then the update's -- and stored once;
//   accept counts          an exact integer sum per team: the wave butterfly, for the workgroup team the LDS cells of the scans; one store per block and
//                          step into acc_out[t][blk], no atomics.  Move-reweight takes every proposal: cnt * n_iters where the block resampled.
// Counters are the loop's: resample slot under E + 3t; the move of particle gid under E + 3t + 1 -- TAG_MOVE, proposal block it (NBLK + 1), uniform
// block + NBLK; TAG_REWEIGHT, block it NBLK --; the propagate under E + 3t + 2, TAG_UPDATE.  has_prev is the handle's at step 0 and true afterwards
// (right after gpf_initialize_blocks the first move re-draws from the prior).  Floating-point order is the loop's: llx is carried across the MH
// iterations, wsum = wsum + (lls - llx), lw = (new_lw + wsum) + ll.
struct RunMoveArgs {
    RunArgs r;                                     // as k_block_run takes them, with W = row_width(D, true) and the epochs three apart
    int32_t n_iters;                               // >= 0
    int32_t has_prev;                              // the handle's on entry
    int64_t* acc_out;                              // [n_steps][nblocks] accepted proposals of the blocks that resampled (0 elsewhere), or null
};
// the exact sum of one count per lane over the team; s_x as in team_scan_incl (TEAM = BLOCK only)
template <int TEAM>
__device__ __forceinline__ uint64_t team_count(uint32_t v, uint64_t (*s_x)[4])
{
    uint64_t t = wave_sum_u64((uint64_t)v);
    if (TEAM == BLOCK) {
        __syncthreads();                                           // (s_x may still be read by the step's scans)
        if (lane_id() == 0) s_x[wave_id()][0] = t;
        __syncthreads();
        t = 0;
#pragma unroll
        for (int w = 0; w < NWAVES; ++w) t += s_x[w][0];
    }
    return t;
}
template <int M, int W, int METHOD, bool REWEIGHT, int TEAM, int ITEMS>    // METHOD as k_block_run; W = row_width(Model<M>::D, true)
__global__ __launch_bounds__(BLOCK) void k_block_run_move(RunMoveArgs am)
{
    using Mo = Model<M>;
    constexpr int D = Mo::D, NB = Mo::NBLK;
    constexpr int TEAMS = BLOCK / TEAM, CAP = TEAM * ITEMS;
    static_assert(TEAM == WAVE || TEAM == BLOCK, "a wave or the workgroup");
    static_assert(W >= 2 * D && W % 2 == 0, "rows [x | x_{t-1}], moved as 16-byte column pairs");
    const RunArgs& a = am.r;
    __shared__ uint64_t s_cdf_[BLOCK * ITEMS];
    __shared__ uint64_t s_aux_[METHOD == 0 ? 1 : BLOCK * ITEMS];
    __shared__ uint16_t s_idx_[METHOD == 2 ? BLOCK * ITEMS : 1];
    __shared__ uint64_t s_x[NWAVES][4];
    __shared__ double s_m[NWAVES];
    __shared__ int s_f[NWAVES];
    const int tm = (int)threadIdx.x / TEAM, tl = (int)threadIdx.x % TEAM;
    const int64_t blk = (int64_t)blockIdx.x * TEAMS + tm;
    if (TEAM != BLOCK && blk >= a.nblocks) return;                 // (an idle wave: the wave-team path has no workgroup barrier)
    uint64_t* const s_cdf = s_cdf_ + tm * CAP;
    uint64_t* const s_aux = s_aux_ + (METHOD == 0 ? 0 : tm * CAP);
    uint16_t* const s_idx = s_idx_ + (METHOD == 2 ? tm * CAP : 0);
    const int64_t b0 = blk * a.nb;
    const int cnt = (int)(a.n - b0 < a.nb ? a.n - b0 : a.nb);
    const int K = fix_K(cnt);
    const double* const P = a.blk_params ? a.blk_params + blk * MAX_PARAMS : a.P;      // (team-uniform; move and propagate alike)
    const double* const obs_b = a.obs + (a.obs_blocks == 1 ? 0 : (size_t)blk * (size_t)a.n_steps * (size_t)a.n_obs);
    const double lml0 = *a.lml_est;
    double* const lw = a.lw + b0;
    double obp[MAX_OBS];                                           // the observation the move conditions on: the block's latest
#pragma unroll
    for (int k = 0; k < MAX_OBS; ++k) obp[k] = a.blk_obs[blk * MAX_OBS + k];
    bool has_prev = am.has_prev != 0;
    int side = 0, flags_all = 0;
    double m; int f; uint64_t q[ITEMS]; uint64_t S_w; double ess;
    run_summary<TEAM, ITEMS>(lw, cnt, K, tl, s_m, s_f, s_x, m, f, q, S_w, ess);
#pragma unroll 1
    for (int t = 0; t < a.n_steps; ++t) {
        // ================ k_block_resample<METHOD>, epoch E + 3t (k_block_run's statements)
        const uint32_t ep_r = a.epoch + 3u * (uint32_t)t, ep_m = ep_r + 1u, ep_u = ep_r + 2u;
        const bool gate = a.ess_frac >= 0.0 ? (f == 0 && ess < a.ess_frac * (double)cnt) : true;
        const bool skip = (f & (FLAG_NAN | FLAG_POSINF)) != 0;
        const bool uniform = (f & FLAG_ALL_NEGINF) != 0;
        const bool go = gate && !skip;
        if (tl == 0) a.res_out[(int64_t)t * a.nblocks + blk] = (go ? 1 : 0) | ((gate ? f : 0) << 8);
        flags_all |= gate ? f : 0;
        uint64_t S = 0, Ctot = 0, Rs = 0;
        if (go) {
            if (METHOD == 2 && a.sorted) {
                int p2 = 2;
                while (p2 < cnt) p2 <<= 1;
                for (int i = tl; i < p2; i += TEAM) { s_aux[i] = i < cnt ? sort_key_desc(lw[i]) : ~0ull; s_idx[i] = (uint16_t)i; }
                team_sync<TEAM>();
                for (int size = 2; size <= p2; size <<= 1) {
                    for (int stride = size >> 1; stride >= 1; stride >>= 1) {
                        for (int e = tl; e < p2 / 2; e += TEAM) {
                            const int lo = 2 * e - (e & (stride - 1)), hi = lo + stride;
                            const bool up = (lo & size) == 0;
                            const uint64_t ka = s_aux[lo], kb = s_aux[hi];
                            const uint16_t ia = s_idx[lo], ib = s_idx[hi];
                            const bool gt = ka > kb || (ka == kb && ia > ib);
                            if (gt == up) { s_aux[lo] = kb; s_aux[hi] = ka; s_idx[lo] = ib; s_idx[hi] = ia; }
                        }
                        team_sync<TEAM>();
                    }
                }
#pragma unroll
                for (int k = 0; k < ITEMS; ++k) {
                    const int i = ITEMS * tl + k;
                    q[k] = i < cnt ? (uniform ? 1ull : exp_fix(sort_key_value(s_aux[i]) - m, K)) : 0ull;
                }
                team_sync<TEAM>();
            }
            if (METHOD == 1) {
                uint64_t sq[ITEMS];
#pragma unroll
                for (int k = 0; k < ITEMS; ++k) sq[k] = q[k];
                S = team_scan_incl<TEAM, ITEMS>(sq, s_x);
                const int sh = residual_shift(S, cnt);
                uint64_t c[ITEMS], r[ITEMS];
#pragma unroll
                for (int k = 0; k < ITEMS; ++k) {
                    const uint64_t nq = (uint64_t)cnt * q[k];
                    uint64_t cq = (uint64_t)((double)nq / (double)S), prod = cq * S;
                    if (prod > nq) { cq -= 1; prod -= S; }
                    uint64_t rq = nq - prod;
                    if (rq >= S) { cq += 1; rq -= S; }
                    c[k] = cq; r[k] = rq >> sh;
                }
                Ctot = team_scan_incl<TEAM, ITEMS>(c, s_x);
                Rs = team_scan_incl<TEAM, ITEMS>(r, s_x);
#pragma unroll
                for (int k = 0; k < ITEMS; ++k) { s_aux[ITEMS * tl + k] = c[k]; s_cdf[ITEMS * tl + k] = r[k]; }
            } else {
                S = team_scan_incl<TEAM, ITEMS>(q, s_x);
#pragma unroll
                for (int k = 0; k < ITEMS; ++k) s_cdf[ITEMS * tl + k] = q[k];
            }
            team_sync<TEAM>();
        }
        const double new_lw = go ? lse_from(m, S, K, f) - log_((double)cnt) : 0.0;
        const uint64_t sB = METHOD == 2 && go ? S / (uint64_t)cnt : 0, srem = METHOD == 2 && go ? S % (uint64_t)cnt : 0;
        // ================ the slots: ancestor, move under E + 3t + 1 and the previous observation, propagate under E + 3t + 2 and this step's
        double ob[MAX_OBS];
        {
            const double* const orow = obs_b + (size_t)t * (size_t)a.n_obs;
#pragma unroll
            for (int k = 0; k < MAX_OBS; ++k) ob[k] = k < a.n_obs ? orow[k] : 0.0;
        }
        const double* const rows_in = a.rows[side] + b0 * W;
        double* const rows_out = a.rows[go ? 1 - side : side] + b0 * W;
        const int iters = go ? am.n_iters : 0;                     // (team-uniform: only the blocks that resampled move)
        uint32_t acc = 0;
        for (int j = tl; j < cnt; j += TEAM) {
            const uint32_t slot = (uint32_t)(a.gid0 + b0 + j);     // the resample's slot, and the particle's RNG counter in move and propagate
            int anc = j;
            if (go) {
                if (METHOD == 0) anc = lds_upper_bound(s_cdf, cnt, mulhi64(resample_u64(a.seed, slot, ep_r), S));
                else if (METHOD == 1) {
                    if ((uint64_t)j < Ctot) anc = lds_upper_bound(s_aux, cnt, (uint64_t)j);
                    else anc = lds_upper_bound(s_cdf, cnt, mulhi64(resample_u64(a.seed, slot, ep_r), Rs));
                } else {
                    const uint64_t jl = (uint64_t)j;
                    const uint64_t L0 = jl * sB + (uint32_t)(jl * srem) / (uint32_t)cnt, L1 = (jl + 1) * sB + (uint32_t)((jl + 1) * srem) / (uint32_t)cnt;
                    anc = lds_upper_bound(s_cdf, cnt, L0 + mulhi64(resample_u64(a.seed, slot, ep_r), L1 - L0));
                    if (a.sorted) anc = (int)s_idx[anc];
                }
                a.anc[b0 + j] = anc;
            }
            // ---- the one load: x and x_{t-1} of the ancestor
            double x[MAX_DIM], xp[MAX_DIM];
            {
                double r[W];
                const double2* src = reinterpret_cast<const double2*>(rows_in + (size_t)anc * W);
#pragma unroll
                for (int c = 0; c < W / 2; ++c) { const double2 v = src[c]; r[2 * c] = v.x; r[2 * c + 1] = v.y; }
#pragma unroll
                for (int k = 0; k < D; ++k) { x[k] = r[k]; xp[k] = r[D + k]; }
            }
            // ---- k_move<M, W, REWEIGHT, false, false, true>'s iterations, on registers
            double wsum = 0.0;
            if (iters > 0) {
                double xs[MAX_DIM];
                double llx = Mo::loglik(P, x, obp);
#pragma unroll 1
                for (int it = 0; it < iters; ++it) {
                    if (REWEIGHT) {
                        Mo::sample(P, !has_prev, xp, obp, a.seed, slot, (uint32_t)(it * NB), ep_m, TAG_REWEIGHT, xs);
                        const double lls = Mo::loglik(P, xs, obp);
                        wsum = wsum + (lls - llx);                                     // rejuvenate.jl:86
#pragma unroll
                        for (int k = 0; k < D; ++k) x[k] = xs[k];
                        llx = lls;
                    } else {
                        const uint32_t blk0 = (uint32_t)(it * (NB + 1));
                        Mo::sample(P, !has_prev, xp, obp, a.seed, slot, blk0, ep_m, TAG_MOVE, xs);
                        const double lls = Mo::loglik(P, xs, obp);
                        const Philox b = rng(a.seed, slot, blk0 + NB, ep_m, TAG_MOVE);
                        const bool ok = log_(u52(b.w0, b.w1)) < lls - llx;             // Gen.mh's accept: a select, no branch
#pragma unroll
                        for (int k = 0; k < D; ++k) x[k] = ok ? xs[k] : x[k];
                        llx = ok ? lls : llx;
                        acc += ok ? 1u : 0u;
                    }
                }
            }
            // ---- k_step's default proposal from the moved x, this step's observation
            double xn[MAX_DIM];
            Mo::sample(P, false, x, ob, a.seed, slot, 0, ep_u, TAG_UPDATE, xn);
            const double ll = Mo::loglik(P, xn, ob);
            double o[W];
#pragma unroll
            for (int k = 0; k < W; ++k) o[k] = 0.0;
#pragma unroll
            for (int k = 0; k < D; ++k) { o[k] = xn[k]; o[D + k] = x[k]; }
            // ---- the one store
            double2* dst = reinterpret_cast<double2*>(rows_out + (size_t)j * W);
#pragma unroll
            for (int c = 0; c < W / 2; ++c) dst[c] = make_double2(o[2 * c], o[2 * c + 1]);
            const double lw_in = go ? (REWEIGHT ? new_lw + wsum : new_lw) : lw[j];
            lw[j] = lw_in + ll;
        }
        if (am.acc_out) {                                          // (kernel-uniform)
            const uint64_t n_acc = REWEIGHT ? (uint64_t)(go ? cnt : 0) * (uint64_t)am.n_iters : team_count<TEAM>(acc, s_x);
            if (tl == 0) am.acc_out[(int64_t)t * a.nblocks + blk] = (int64_t)n_acc;
        }
        if (go) side ^= 1;
        has_prev = true;
#pragma unroll
        for (int k = 0; k < MAX_OBS; ++k) obp[k] = ob[k];
        run_sync<TEAM>();
        // ================ k_block_stats: step t's outputs, step t + 1's gate and weights
        run_summary<TEAM, ITEMS>(lw, cnt, K, tl, s_m, s_f, s_x, m, f, q, S_w, ess);
        if (tl == 0) {
            a.ess_out[(int64_t)t * a.nblocks + blk] = f ? __builtin_nan("") : ess;
            a.lml_out[(int64_t)t * a.nblocks + blk] = (lml0 + lse_from(m, S_w, K, f)) - log_((double)cnt);
        }
    }
    if (tl == 0) a.flags_out[blk] = flags_all << 8;
    if (tl < MAX_OBS)                                              // the handle's per-block observation row: the last step's
        a.blk_obs[blk * MAX_OBS + tl] = tl < a.n_obs ? obs_b[(size_t)(a.n_steps - 1) * (size_t)a.n_obs + tl] : 0.0;
    if (side)
        for (int e = tl; e < cnt * (W / 2); e += TEAM)
            reinterpret_cast<double2*>(a.rows[0] + b0 * W)[e] = reinterpret_cast<const double2*>(a.rows[1] + b0 * W)[e];
}

} // namespace gpf
