// K11h: a particle Gibbs chain per block in one launch  (part of gpf_kernels.hpp; include that header, not this file)
#pragma once

namespace gpf {
// ----------------------------------------------------------------------------- sweep, take the drawn path as the retained one, sweep again: per block
// gpf_gibbs_blocks (gpf.h): the chain particle Gibbs runs (Andrieu, Doucet & Holenstein 2010; with ancestor sampling Lindsten, Jordan &
// Schoen 2014; with backward simulation Whiteley 2010, Lindsten & Schoen 2013) -- PGAS used as a smoother is the same chain --
//     for k in 1:K
//         twin = a fresh filter of this size and model under seeds[k];  gpf_initialize_blocks_ref(twin, obs[:, 0], ref[:, 0])       epoch 0
//         gpf_sweep_blocks[_backward](twin, obs[:, 1:], ref[:, 1:]) -> path, lml[:, k] = its last step's                            epochs 1 ..
//         ref = path;  k % thin == 0: paths[:, k / thin] = path
//     end
// in ONE launch.  No twin exists: team b (team_dispatch) runs all K sweeps of block b -- K T steps and K path draws -- with no launch and no host in
// between, and the retained path never leaves the device.  Per sweep:
//   prologue   the body of k_init<M, MODE_REF, true, BP> for the block's slots under (seeds[k], epoch 0, TAG_INIT), RNG counter gid0 + b0 + j: every
//              lane draws, slot 0's latent is overwritten by cur[b][0] and weighted by its loglik (gpf_k_block_pmmh.hpp shows this prologue without
//              the pin).  The rows go straight into slab 0, the weights into the call's [n] doubles: nothing of the handle is read or written;
//   steps      t = 1 .. T-1: k_block_sweep's step restated (gpf_k_block_sweep.hpp, where every statement is explained) through the same helpers in the
//              same order -- the gate from the closing summary, the ancestor weights / CDF / team-uniform search for a_0 where AS, the weight CDF, the
//              slots, run_sync, run_summary; BACK: one more 8-byte weight store per slot.  The twin's sweep starts at epoch 1: step t resamples under
//              1 + 2(t-1) and propagates under 2 + 2(t-1).  xr of step t is cur[b][t], a team-uniform broadcast row.  The same sums: the same bits;
//   lml        (0 + lse(final weights)) - log(cnt): k_block_stats on a fresh twin, whose log_ml_est is the +0.0 of after_initialize.  The per-step
//              ess / lml / resampled of the sweep are not formed (the resample word is kept: the tail reads it);
//   tail       k_block_sweep's, the draw under epoch 1 + 2(T-1) (BACK: and the T-1 epochs behind it): lane 0's ancestral walk or the whole team's
//              backward pass.  It reads rows only from the slabs and writes the path over cur[b] -- and, on a kept sweep, into paths[b][kept] --: the
//              hand-over of the retained path is in place.  In the ancestral tail the other lanes wait at the sync below; they do not return;
//   hand-over  ONE run_sync between the tail's last store and the next prologue's first load of cur[b].
// Scratch is the sweep's and does not grow with K: slabs = [T][n][W] rows, par = [T-1][n] 16-bit block-local parents, res = [T-1][nblocks] resample words,
// BACK: lws = [T-1][n] weights -- every sweep overwrites the previous one's (the sync of the hand-over orders the tail's loads before the prologue's
// stores).  cur = [nblocks][T][D], uploaded once.
// A block whose sweep ends with NaN / +Inf weights -- the loop would refuse its NaN path as the next reference -- reads NaN in that sweep's and every
// later kept path and lml entry and does no further work: the decision is team-uniform (the flags are), so the whole team leaves together.
// LDS: s_cdf and the reduction cells, the sweep's.  Synchronisation: run_sync / team_sync exactly as argued in gpf_k_block_run.hpp and the sweep; no spin
// waits, nothing between workgroups; every loop is bounded by K, T, cnt or log2 cnt.
struct GibbsArgs {
    double* slabs;                                 // [T][n][W]
    uint16_t* par;                                 // [T - 1][n] parents, local to the block, of the steps in which the block resampled
    int32_t* res;                                  // [T - 1][nblocks] the word of step t's resample: bit 0 is what the tail reads
    double* lws;                                   // BACK: [T - 1][n] what slot j enters step t's propagate with
    double* lw;                                    // [n] the current weights
    double* cur;                                   // [nblocks][T][D] the retained paths: the caller's on entry, sweep k's draw behind sweep k
    int64_t n, nb, nblocks, gid0;
    const uint64_t* seeds;                         // [K] one per sweep
    int32_t n_sweeps, thin, n_kept;                // K; every thin-th path is kept: n_kept = K / thin
    int32_t n_steps;                               // T: the whole series, the initial step included (>= 2)
    double ess_frac;                               // < 0: every block resamples at every step
    const double* P;                               // [MAX_PARAMS] the filter's parameters (device)
    const double* blk_params;                      // [nblocks][MAX_PARAMS] or null
    const double* obs; int64_t obs_blocks;         // [obs_blocks][T][n_obs], the caller's layout; obs_blocks = nblocks | 1
    int32_t n_obs;
    double* paths;                                 // [nblocks][n_kept][T][D]
    double* lml;                                   // [nblocks][K]
};
template <int M, int W, bool AS, int TEAM, int ITEMS, bool BACK>    // W = row_width(Model<M>::D, false); BACK: the paths by backward simulation
__global__ __launch_bounds__(BLOCK) void k_block_gibbs(GibbsArgs a)
{
    using Mo = Model<M>;
    constexpr int D = Mo::D;
    constexpr int TEAMS = BLOCK / TEAM, CAP = TEAM * ITEMS;        // blocks per workgroup, particles a team holds
    static_assert(TEAM == WAVE || TEAM == BLOCK, "a wave or the workgroup");
    static_assert(W >= D && W % 2 == 0, "rows are moved as 16-byte column pairs");
    static_assert(D == 1 || D % 2 == 0, "the path is written as words or 16-byte pairs");
    static_assert(BLK_MAX <= 65536, "16-bit parents");
    __shared__ uint64_t s_cdf_[BLOCK * ITEMS];                     // the ancestor weights' CDF (AS), then the weights'; in the tail the draw's (BACK: and every backward step's)
    __shared__ uint64_t s_x[NWAVES][4];
    __shared__ double s_m[NWAVES];
    __shared__ int s_f[NWAVES];
    const int tm = (int)threadIdx.x / TEAM, tl = (int)threadIdx.x % TEAM;
    const int64_t blk = (int64_t)blockIdx.x * TEAMS + tm;
    if (TEAM != BLOCK && blk >= a.nblocks) return;                 // (an idle wave: the wave-team path has no workgroup barrier)
    uint64_t* const s_cdf = s_cdf_ + tm * CAP;
    const int64_t b0 = blk * a.nb;
    const int cnt = (int)(a.n - b0 < a.nb ? a.n - b0 : a.nb);      // particles of this block (<= CAP: team_dispatch)
    const int K = fix_K(cnt);
    const int T = a.n_steps, ns = T - 1;                           // ns: the steps of one sweep
    const double* const P = a.blk_params ? a.blk_params + blk * MAX_PARAMS : a.P;      // (team-uniform)
    const double* const obs_b = a.obs + (a.obs_blocks == 1 ? 0 : (size_t)blk * (size_t)T * (size_t)a.n_obs);              // the block's series
    double* const cur_b = a.cur + (size_t)blk * (size_t)T * D;                                                            // ... and retained path
    double* const paths_b = a.paths + (size_t)blk * (size_t)a.n_kept * (size_t)T * D;
    double* const lml_b = a.lml + (size_t)blk * (size_t)a.n_sweeps;
    double* const lw = a.lw + b0;
    const size_t slab = (size_t)a.n * W;                           // doubles per slab
    const double logc = log_((double)cnt);
    auto obs_row = [&](int t, double (&ob)[MAX_OBS]) {             // the block's row of step t, zero-padded as the staged rows of gpf_update_blocks
        const double* const orow = obs_b + (size_t)t * (size_t)a.n_obs;
#pragma unroll
        for (int k = 0; k < MAX_OBS; ++k) ob[k] = k < a.n_obs ? orow[k] : 0.0;
    };
#pragma unroll 1
    for (int sw = 0; sw < a.n_sweeps; ++sw) {
        const uint64_t seed = a.seeds[sw];                         // (team-uniform)
        const int kept = (sw + 1) % a.thin == 0 ? (sw + 1) / a.thin - 1 : -1;
        double* const keep = kept >= 0 ? paths_b + (size_t)kept * (size_t)T * D : nullptr;
        // ================ prologue: k_init<M, MODE_REF> under the twin's epoch 0, the rows straight into slab 0
        {
            double ob[MAX_OBS], xr[D];
            obs_row(0, ob);
#pragma unroll
            for (int k = 0; k < D; ++k) xr[k] = cur_b[k];
            double* const rows0 = a.slabs + b0 * W;
            for (int j = tl; j < cnt; j += TEAM) {
                double x[MAX_DIM];
                Mo::sample(P, true, nullptr, ob, seed, (uint32_t)(a.gid0 + b0 + j), 0, 0u, TAG_INIT, x);
#pragma unroll
                for (int k = 0; k < D; ++k) x[k] = j == 0 ? xr[k] : x[k];        // (every lane draws; the pinned lane overwrites its draw)
                const double ll = Mo::loglik(P, x, ob);
                double o[W];
#pragma unroll
                for (int k = 0; k < W; ++k) o[k] = 0.0;
#pragma unroll
                for (int k = 0; k < D; ++k) o[k] = x[k];
                double2* dst = reinterpret_cast<double2*>(rows0 + (size_t)j * W);
#pragma unroll
                for (int c = 0; c < W / 2; ++c) dst[c] = make_double2(o[2 * c], o[2 * c + 1]);
                lw[j] = ll;
            }
        }
        run_sync<TEAM>();
        double m; int f; uint64_t q[ITEMS]; uint64_t S_w; double ess;
        run_summary<TEAM, ITEMS>(lw, cnt, K, tl, s_m, s_f, s_x, m, f, q, S_w, ess);
        // ================ steps 1 .. T-1: k_block_sweep's step; the twin's sweep starts at epoch 1
#pragma unroll 1
        for (int t = 0; t < ns; ++t) {
            const uint32_t ep_r = 1u + 2u * (uint32_t)t, ep_u = ep_r + 1u;
            const bool gate = a.ess_frac >= 0.0 ? (f == 0 && ess < a.ess_frac * (double)cnt) : true;
            const bool skip = (f & (FLAG_NAN | FLAG_POSINF)) != 0;     // NaN / +Inf: left as it stands (check = false)
            const bool go = gate && !skip;
            if (tl == 0) a.res[(int64_t)t * a.nblocks + blk] = go ? 1 : 0;
            double ob[MAX_OBS], xr[D];                                 // (team-uniform: the block's rows of step t + 1 of the series)
            obs_row(t + 1, ob);
            {
                const double* const rrow = cur_b + (size_t)(t + 1) * D;
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
                    if (f_a == 0) a0 = lds_upper_bound(s_cdf, cnt, mulhi64(resample_u64(seed, (uint32_t)(a.gid0 + b0), ep_r), S_a));
                    team_sync<TEAM>();                                 // (s_cdf is overwritten next)
                }
                S = team_scan_incl<TEAM, ITEMS>(q, s_x);
#pragma unroll
                for (int k = 0; k < ITEMS; ++k) s_cdf[ITEMS * tl + k] = q[k];
                team_sync<TEAM>();
            }
            const double new_lw = go ? lse_from(m, S, K, f) - logc : 0.0;
            // ---- the slots: ancestor, then k_step's MODE_REF body under the epoch behind the resample's
            for (int j = tl; j < cnt; j += TEAM) {                     // consecutive lanes, consecutive slots: coalesced stores
                const uint32_t slot = (uint32_t)(a.gid0 + b0 + j);
                int anc = j;
                if (go) {
                    anc = lds_upper_bound(s_cdf, cnt, mulhi64(resample_u64(seed, slot, ep_r), S));
                    if (j == 0) anc = a0;                              // the retained path
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
                Mo::sample(P, false, r, ob, seed, slot, 0, ep_u, TAG_UPDATE, xn);
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
            run_summary<TEAM, ITEMS>(lw, cnt, K, tl, s_m, s_f, s_x, m, f, q, S_w, ess);
        }
        // ================ the sweep's estimate; a block with NaN / +Inf final weights ends here (team-uniform)
        if ((f & (FLAG_NAN | FLAG_POSINF)) != 0) {
            for (int e = tl; e < a.n_sweeps - sw; e += TEAM) lml_b[sw + e] = __builtin_nan("");
            const int k0 = (sw + 1 + a.thin - 1) / a.thin - 1;         // the first kept path at or behind this sweep
            for (int64_t e = (int64_t)k0 * T * D + tl; e < (int64_t)a.n_kept * T * D; e += TEAM) paths_b[e] = __builtin_nan("");
            return;
        }
        if (tl == 0) lml_b[sw] = (0.0 + lse_from(m, S_w, K, f)) - logc;    // k_block_stats on the twin: (log_ml_est + logsumexp) - log(cnt), left to right
        const uint32_t ep_d = 1u + 2u * (uint32_t)ns;
        const uint64_t S_d = team_scan_incl<TEAM, ITEMS>(q, s_x);
#pragma unroll
        for (int k = 0; k < ITEMS; ++k) s_cdf[ITEMS * tl + k] = q[k];
        team_sync<TEAM>();
        if constexpr (!BACK) {
            // ================ k_block_sample_traj with n_samples = 1: the draw from the final weights, lane 0's walk down the slabs
            if (tl == 0) {
                int p = lds_upper_bound(s_cdf, cnt, mulhi64(resample_u64(seed, (uint32_t)blk, ep_d), S_d));
                for (int s = ns; s >= 0; --s) {
                    const double* const x = a.slabs + (size_t)s * slab + (size_t)(b0 + p) * W;
                    double* const o = cur_b + (size_t)s * D;
                    if constexpr (D == 1) { const double v = x[0]; o[0] = v; if (keep) keep[s] = v; }
                    else {
#pragma unroll
                        for (int c = 0; c < D / 2; ++c) {
                            const double2 v = reinterpret_cast<const double2*>(x)[c];
                            reinterpret_cast<double2*>(o)[c] = v;
                            if (keep) reinterpret_cast<double2*>(keep + (size_t)s * D)[c] = v;
                        }
                    }
                    if (s > 0 && (a.res[(int64_t)(s - 1) * a.nblocks + blk] & 1)) p = (int)a.par[(size_t)(s - 1) * (size_t)a.n + b0 + p];
                }
            }
        } else {
            // ================ k_block_backward with n_samples = 1: the draw from the final weights, then the whole team per step down the slabs
            int p = lds_upper_bound(s_cdf, cnt, mulhi64(resample_u64(seed, (uint32_t)blk, ep_d), S_d));      // (team-uniform, local to the block)
            team_sync<TEAM>();                                         // (s_cdf is overwritten next)
            int go_s = 0;                                              // (the last step stands as its propagate left it: r = the identity)
#pragma unroll 1
            for (int s = ns; ; --s) {
                // the recorded parent of the held particle -- a 16-bit load where the block resampled in iteration s -- is its row in slab s
                const int pm = go_s ? (int)a.par[(size_t)s * (size_t)a.n + b0 + p] : p;
                const double* __restrict__ xh = a.slabs + (size_t)s * slab + (size_t)(b0 + pm) * W;    // one broadcast address
                double xr[D];
                load_latent<D>(xh, xr);
                if (tl == 0) {
#pragma unroll
                    for (int k = 0; k < D; ++k) { cur_b[(size_t)s * D + k] = xr[k]; if (keep) keep[(size_t)s * D + k] = xr[k]; }
                }
                if (s == 0) break;
                go_s = a.res[(int64_t)(s - 1) * a.nblocks + blk] & 1;  // (team-uniform) iteration s - 1: the order of the candidates
                double ob[MAX_OBS];
                obs_row(s, ob);                                        // (the series at iteration s - 1 of the sweep: row s of the whole series)
                const double* __restrict__ plw = a.lws + (size_t)(s - 1) * (size_t)a.n + b0;
                const uint16_t* __restrict__ par = a.par + (size_t)(s - 1) * (size_t)a.n + b0;
                const double* __restrict__ rows_c = a.slabs + (size_t)(s - 1) * slab + b0 * W;
                double lwa[ITEMS];
#pragma unroll
                for (int k = 0; k < ITEMS; ++k) {                      // anc_weights, the candidate's row gathered through its parent
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
                if (f_a == 0) p = lds_upper_bound(s_cdf, cnt, mulhi64(resample_u64(seed, (uint32_t)blk, ep_d + (uint32_t)(ns - s + 1)), S_a));
                team_sync<TEAM>();                                     // (s_cdf is overwritten by the next step)
            }
        }
        run_sync<TEAM>();                                              // the hand-over: the path is the next sweep's retained one, the slabs are free again
    }
}

} // namespace gpf
