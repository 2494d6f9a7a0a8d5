// K11b: backward simulation per block from the trajectory store  (part of gpf_kernels.hpp; include that header, not this file)
#pragma once

namespace gpf {
// ----------------------------------------------------------------------------- what the store records for a backward pass
// gpf_history_enable_blocks_weights: beside a step's latent columns (k_hist_snapshot) its n log-weights and the [n_blocks][MAX_OBS] observation rows
// it was entered with, as they stand at the snapshot -- one launch for both.  n_obs_words = 0: a step entered by a whole-filter call (no rows).
static __global__ __launch_bounds__(BLOCK) void k_hist_record(const double* __restrict__ lw, int64_t n, const double* __restrict__ obs, int64_t n_obs_words,
                                                              double* __restrict__ lw_out, double* __restrict__ obs_out)
{
    const int64_t gt = (int64_t)blockIdx.x * BLOCK + threadIdx.x, gs = (int64_t)gridDim.x * BLOCK;
    for (int64_t i = gt; i < n; i += gs) lw_out[i] = lw[i];
    for (int64_t i = gt; i < n_obs_words; i += gs) obs_out[i] = obs[i];
}

// ----------------------------------------------------------------------------- backward simulation, block by block
// gpf_block_backward_sample (gpf.h; Godsill, Doucet & West 2004, "Monte Carlo smoothing for nonlinear time series", JASA 99; as the path draw of
// particle Gibbs: Whiteley 2010, Lindsten & Schoen 2013): draw j of block b is a path x_1:T whose step-T particle is drawn from the block's current
// weights -- exactly k_block_sample_traj's draw -- and whose particle at every earlier step s is drawn among the particles of snapshot s from
//     P(i)  proportional to  w_s^i f(x_{s+1} | x_s^i),          x_{s+1} = the particle the draw holds at step s + 1,
// instead of being the recorded parent.  ONE launch for all blocks, draws and steps; the team works on one (draw, step) pair at a time:
//   step T     the block's weight CDF in s_cdf (from the lane's registers: every draw restores it), a = upper_bound(cdf, mulhi64(U, S)),
//              U = resample_u64(seed, slot, epoch), slot = b n_samples + j;
//   step s     (0-based q -> q - 1 below) p = the held particle in the final order of step q, pm = maps[q][p] its recorded parent (p where the step had
//              no resample), c = pm / nb the block it was born from -- b itself unless a resample across blocks moved the lineage.  Candidates: the
//              particles of block c in snapshot q - 1, ITEMS per lane; lwa_i = hist_lw[q-1][i] + logtrans(P_b, hist_x[q-1][i], hist_x[q][p],
//              hist_obs[q][p / nb]) (anc_weights of gpf_k_block_anc.hpp; the held particle's columns and the observation row are one broadcast address);
//              then k_block_resample_anc's statements: team_max_flags, K = fix_K(cnt of block c), exp_fix(lwa - m', K), the inclusive scan into s_cdf,
//              a = upper_bound(cdf, mulhi64(U_q, S')) with U_q = resample_u64(seed, slot, epoch + (T - q)); new p = c nb + a.
//   fallback   flags of lwa hold NaN, +Inf or ALL_NEGINF -> p = pm, the ancestral step.
//   bad block  current weights with NaN / +Inf: indices 0 and NaN paths, as k_block_sample_traj.
// P_b: block b's row of blk_params where per-block parameters are set (they travel with their block: the lineage's parameters), else the filter's.
// Outputs: traj = [nblocks][n_samples][hi0 - lo0 + 1][D], idx (may be null) = [nblocks][n_samples][hi0 - lo0 + 1] 1-based GLOBAL indices in the step's
// final order; steps above hi0 are walked, not written.  Lane 0 of the team writes.  The draws of a block are independent, so gridDim.y splits them
// (draw j goes to the workgroups with blockIdx.y = j mod gridDim.y): few large blocks with many draws still fill the machine.
// LDS is k_block_sample_traj's.  The two syncs around every search of s_cdf are needed: the next (draw, step) overwrites it.
struct BackArgs {
    const int32_t* const* maps;                    // [T] composed ancestor maps, nullptr = no resample in that step
    const double* const* hx;                       // [T] snapshots [n][D]
    const double* const* hlw;                      // [T] recorded log-weights [n]
    const double* const* hobs;                     // [T] recorded observation rows [nblocks][MAX_OBS]
    const double* lw;                              // the current log-weights
    int T, lo0, hi0, n_samples;
    int64_t n, nb, nblocks;
    uint64_t seed; uint32_t epoch;
    double* traj; int64_t* idx;
};
template <int M, int TEAM, int ITEMS>
__global__ __launch_bounds__(BLOCK) void k_block_backward(BackArgs a, AncArgs x)
{
    using Mo = Model<M>;
    constexpr int D = Mo::D;
    constexpr int TEAMS = BLOCK / TEAM, CAP = TEAM * ITEMS;
    static_assert(TEAM == WAVE || TEAM == BLOCK, "a wave or the workgroup");
    static_assert(D == 1 || D == 2 || D == 4, "the latent columns are moved as words or 16-byte pairs");
    __shared__ uint64_t s_cdf_[BLOCK * ITEMS];
    __shared__ uint64_t s_x[NWAVES][4];
    __shared__ double s_m[NWAVES];
    __shared__ int s_f[NWAVES];
    const int tm = (int)threadIdx.x / TEAM, tl = (int)threadIdx.x % TEAM;
    const int64_t blk = (int64_t)blockIdx.x * TEAMS + tm;
    if (TEAM != BLOCK && blk >= a.nblocks) return;                 // (an idle wave: the wave-team path has no workgroup barrier)
    uint64_t* const s_cdf = s_cdf_ + tm * CAP;
    const int64_t b0 = blk * a.nb;
    const int cnt = (int)(a.n - b0 < a.nb ? a.n - b0 : a.nb);
    const int n_steps = a.hi0 - a.lo0 + 1;
    // ---- step T: the weight CDF of k_block_sample_traj, statement for statement; q stays in the lane's registers
    double lwv[ITEMS];
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) { const int i = ITEMS * tl + k; lwv[k] = i < cnt ? a.lw[b0 + i] : -__builtin_huge_val(); }
    double m; int f;
    team_max_flags<TEAM, ITEMS>(lwv, tl, cnt, s_m, s_f, m, f);
    uint64_t q[ITEMS];
    {
        const int K = fix_K(cnt);
#pragma unroll
        for (int k = 0; k < ITEMS; ++k) q[k] = ITEMS * tl + k < cnt ? ((f & FLAG_ALL_NEGINF) ? 1ull : exp_fix(lwv[k] - m, K)) : 0ull;
    }
    const uint64_t S = team_scan_incl<TEAM, ITEMS>(q, s_x);
    const bool bad = (f & (FLAG_NAN | FLAG_POSINF)) != 0;          // (team-uniform)
    for (int j = (int)blockIdx.y; j < a.n_samples; j += (int)gridDim.y) {     // (team-uniform: every lane walks the same draw)
        const int64_t draw = blk * a.n_samples + j;                // < 2^31 (checked by the host): the draw's resample slot
        double* const out = a.traj + draw * n_steps * D;
        int64_t* const iout = a.idx ? a.idx + draw * n_steps : nullptr;
        if (bad) {
            for (int t = tl; t < n_steps * D; t += TEAM) out[t] = __builtin_nan("");
            if (iout) for (int t = tl; t < n_steps; t += TEAM) iout[t] = 0;
            continue;
        }
#pragma unroll
        for (int k = 0; k < ITEMS; ++k) s_cdf[ITEMS * tl + k] = q[k];
        team_sync<TEAM>();
        int64_t p = b0 + lds_upper_bound(s_cdf, cnt, mulhi64(resample_u64(a.seed, (uint32_t)draw, a.epoch), S));
        team_sync<TEAM>();                                         // (s_cdf is overwritten next)
        for (int s = a.T - 1; ; --s) {
            const double* __restrict__ xh = a.hx[s] + p * D;       // the held particle of step s: one broadcast address
            if (s <= a.hi0 && tl == 0) {
                double* const o = out + (s - a.lo0) * D;
                if constexpr (D == 1) o[0] = xh[0];
                else {
#pragma unroll
                    for (int c = 0; c < D / 2; ++c) reinterpret_cast<double2*>(o)[c] = reinterpret_cast<const double2*>(xh)[c];
                }
                if (iout) iout[s - a.lo0] = p + 1;
            }
            if (s == a.lo0) break;
            const int32_t* __restrict__ g = a.maps[s];             // (kernel-uniform)
            const int64_t pm = g ? (int64_t)g[p] : p;
            const int64_t c = (int64_t)((uint32_t)pm / (uint32_t)a.nb), c0 = c * a.nb;
            const int ccnt = (int)(a.n - c0 < a.nb ? a.n - c0 : a.nb);
            const int K = fix_K(ccnt);
            double xr[D], ob[MAX_OBS];
            load_latent<D>(xh, xr);
            const double* __restrict__ orow = a.hobs[s] + (size_t)((uint32_t)p / (uint32_t)a.nb) * MAX_OBS;
#pragma unroll
            for (int k = 0; k < MAX_OBS; ++k) ob[k] = orow[k];
            const double* __restrict__ plw = a.hlw[s - 1] + c0;
            double lwc[ITEMS], lwa[ITEMS];
#pragma unroll
            for (int k = 0; k < ITEMS; ++k) { const int i = ITEMS * tl + k; lwc[k] = i < ccnt ? plw[i] : -__builtin_huge_val(); }
            if (x.blk_params) anc_weights<M, D, ITEMS>(x.blk_params + blk * MAX_PARAMS, a.hx[s - 1] + c0 * D, ccnt, tl, xr, ob, lwc, lwa);   // (team-uniform)
            else anc_weights<M, D, ITEMS>(x.P, a.hx[s - 1] + c0 * D, ccnt, tl, xr, ob, lwc, lwa);
            double m_a; int f_a;
            team_max_flags<TEAM, ITEMS>(lwa, tl, ccnt, s_m, s_f, m_a, f_a);
            uint64_t qa[ITEMS];
#pragma unroll
            for (int k = 0; k < ITEMS; ++k) qa[k] = ITEMS * tl + k < ccnt ? exp_fix(lwa[k] - m_a, K) : 0ull;
            const uint64_t S_a = team_scan_incl<TEAM, ITEMS>(qa, s_x);
#pragma unroll
            for (int k = 0; k < ITEMS; ++k) s_cdf[ITEMS * tl + k] = qa[k];
            team_sync<TEAM>();
            // every lane evaluates the draw (a team-uniform search of LDS); invalid ancestor weights: the recorded parent
            p = pm;
            if (f_a == 0) p = c0 + lds_upper_bound(s_cdf, ccnt, mulhi64(resample_u64(a.seed, (uint32_t)draw, a.epoch + (uint32_t)(a.T - s)), S_a));
            team_sync<TEAM>();                                     // (s_cdf is overwritten by the next step or draw)
        }
    }
}

} // namespace gpf
