// K11g: the particle-marginal MH move per block in one launch  (part of gpf_kernels.hpp; include that header, not this file)
#pragma once

namespace gpf {
// ----------------------------------------------------------------------------- propose, filter again from the prior, compare, replace: per block
// gpf_pmmh_blocks (gpf.h): the step SMC^2, parallel particle-marginal MH and a likelihood surface over a parameter grid repeat,
//     twin = a fresh filter of this size and model under `seed` with the proposed parameter rows
//     gpf_initialize_blocks(twin, obs[:, 0]);  gpf_run_blocks(twin, obs[:, 1:])                            epochs 0, then 1 + 2(t-1) and 2 + 2(t-1)
//     Lp[b] = gpf_block_stats(twin).lml[b];  accepted[b] = Lp[b] > log_threshold[b]
//     accepted blocks: rows, parents, parameter row, observation row of the state's block <- the twin's; log-weights <- the twin's (+ the mass shift)
// in ONE launch.  The twin exists only inside the launch: team b (team_dispatch) runs the whole proposal filter of block b and then decides.
//   prologue   the body of k_init<M, 0, true, true> for the block's slots: Model<M>::sample(first = true) under epoch 0, TAG_INIT, RNG counter
//              gid0 + b0 + j -- what a fresh handle of the same size gives its particle --, loglik of obs[b][0], lw = ll, parent = b0 + j (k_iota);
//   series     steps 1 .. T-1: k_block_series<.., RunPlain>'s step restated (gpf_k_block_run.hpp, where every statement is explained): the summary the
//              previous step closed with is the gate and the weights of this step's resample, the ESS gate, the optional bitonic order, the CDF(s) in
//              LDS, the search of slot gid0 + b0 + j under epoch 1 + 2(t-1), the ancestor's row straight into Model<M>::sample under the epoch behind
//              it, the summary of the new weights.  Same helpers (run_summary, team_scan_incl, lds_upper_bound), same order: the same bits;
//   epilogue   Lp = (0 + lse(twin weights)) - log(cnt), k_block_stats' value on the twin (whose log_ml_est is the +0.0 of after_initialize); the
//              decision is team-uniform: every operand is.  keep_mass: the summary of the STATE's block weights gives the one double
//              shift = lme_state - lme_twin with lme = lse - log(cnt), added per particle -- the lw + (M - L[a]) of k_block_gather: the block keeps the
//              mass it stands for at the outer level and takes the proposal's inner weights.  A twin with invalid final weights (any flag) is never
//              accepted; with keep_mass a state block with invalid weights is never replaced.  Only an accepted block writes to the handle's buffers:
//              rows, weights, parents in one pass over its slots, its parameter row and its observation row (the last step's, zero-padded) by the
//              first lanes.  A rejected block writes its two output words and nothing else.
// Where the twin lives.  Two row buffers, the log-weights and the parents of the block are the team's own for the whole launch and nothing outside it ever
// looks at them.  IN_LDS (pmmh_in_lds): where the workgroup's teams hold all of that beside the CDFs within 64 KB -- two workgroups and more per compute
// unit -- they are LDS arrays, and the launch's only global traffic is the observations, the parameter row, the two output words and the epilogue of an
// accepted block.  Otherwise they are the call's device scratch (PmmhArgs::s*), ping-ponged as k_block_series ping-pongs the handle's row buffers.
// The arithmetic and the order of every sum are the same statements either way: the same bits.
// Synchronisation: IN_LDS -- team_sync (for the wave team LDS operations execute in order, the fences keep the compiler from moving them);
// scratch -- run_sync, as in k_block_series: data crosses lanes through global memory.  No spin waits, nothing between workgroups, every loop bounded
// by n_steps, cnt or the network's size.
struct PmmhArgs {
    // ---- the state: read for the mass shift, written by accepted blocks only
    double* rows;                                  // [n][W] the handle's current row buffer
    double* lw;                                    // [n]
    int32_t* anc;                                  // [n] parents
    double* blk_params;                            // [nblocks][MAX_PARAMS] the per-block parameter rows in force
    double* blk_obs;                               // [nblocks][MAX_OBS] the per-block observation rows
    // ---- the twin where it does not live in LDS: the call's scratch
    double* srows;                                 // [2][n][W]
    double* slw;                                   // [n]
    int32_t* spar;                                 // [n]
    int64_t n, nb, nblocks, gid0;
    uint64_t seed;                                 // the proposal filter's
    int32_t n_steps;                               // T: the whole series, the initial step included
    int sorted;                                    // stratified: sort_particles
    double ess_frac;                               // < 0: every block resamples at every step
    const double* params;                          // [nblocks][MAX_PARAMS] the proposed rows, zero-padded
    const double* obs; int64_t obs_blocks;         // [obs_blocks][n_steps][n_obs], the caller's layout; obs_blocks = nblocks | 1
    int32_t n_obs;
    const double* thr;                             // [nblocks] log-thresholds (no NaN)
    int keep_mass;
    int32_t* acc_out; double* lml_out;             // [nblocks]
};
// the twin's rows, weights and parents beside the CDF, the copy-count CDF / sort keys and the order, per particle slot of the workgroup
template <int W, int ITEMS>
constexpr bool pmmh_in_lds() { return BLOCK * ITEMS * (2 * W * 8 + 8 + 4 + 8 + 8 + 2) <= 64 * 1024; }

// METHOD 0 multinomial, 1 residual, 2 stratified; W = row_width(Model<M>::D, false)
template <int M, int W, int METHOD, int TEAM, int ITEMS>
__global__ __launch_bounds__(BLOCK) void k_block_pmmh(PmmhArgs a)
{
    using Mo = Model<M>;
    constexpr int D = Mo::D;
    constexpr int TEAMS = BLOCK / TEAM, CAP = TEAM * ITEMS;
    constexpr bool IN_LDS = pmmh_in_lds<W, ITEMS>();
    static_assert(TEAM == WAVE || TEAM == BLOCK, "a wave or the workgroup");
    static_assert(W >= D && W % 2 == 0, "rows are moved as 16-byte column pairs");
    __shared__ uint64_t s_cdf_[BLOCK * ITEMS];
    __shared__ uint64_t s_aux_[METHOD == 0 ? 1 : BLOCK * ITEMS];
    __shared__ uint16_t s_idx_[METHOD == 2 ? BLOCK * ITEMS : 1];
    __shared__ uint64_t s_x[NWAVES][4];
    __shared__ double s_m[NWAVES];
    __shared__ int s_f[NWAVES];
    __shared__ __attribute__((aligned(16))) double s_rows_[IN_LDS ? 2 * BLOCK * ITEMS * W : 2];   // [team][2][CAP][W]
    __shared__ double s_lw_[IN_LDS ? BLOCK * ITEMS : 1];
    __shared__ int32_t s_par_[IN_LDS ? BLOCK * ITEMS : 1];
    const int tm = (int)threadIdx.x / TEAM, tl = (int)threadIdx.x % TEAM;
    const int64_t blk = (int64_t)blockIdx.x * TEAMS + tm;
    if (TEAM != BLOCK && blk >= a.nblocks) return;                 // (an idle wave: the wave-team path has no workgroup barrier)
    uint64_t* const s_cdf = s_cdf_ + tm * CAP;
    uint64_t* const s_aux = s_aux_ + (METHOD == 0 ? 0 : tm * CAP);
    uint16_t* const s_idx = s_idx_ + (METHOD == 2 ? tm * CAP : 0);
    const int64_t b0 = blk * a.nb;
    const int cnt = (int)(a.n - b0 < a.nb ? a.n - b0 : a.nb);      // particles of this block (<= CAP: team_dispatch)
    const int K = fix_K(cnt);
    const double* const P = a.params + blk * MAX_PARAMS;           // the proposed row (team-uniform)
    const double* const obs_b = a.obs + (a.obs_blocks == 1 ? 0 : (size_t)blk * (size_t)a.n_steps * (size_t)a.n_obs);
    // ---- the twin: rows of buffer `side` at rbase + side * rstride
    double* rbase; size_t rstride; double* lw; int32_t* par;
    if constexpr (IN_LDS) { rbase = s_rows_ + (size_t)tm * 2 * CAP * W; rstride = (size_t)CAP * W; lw = s_lw_ + tm * CAP; par = s_par_ + tm * CAP; }
    else { rbase = a.srows + b0 * W; rstride = (size_t)a.n * W; lw = a.slw + b0; par = a.spar + b0; }
    auto twin_sync = [] { if constexpr (IN_LDS) team_sync<TEAM>(); else run_sync<TEAM>(); };
    auto obs_row = [&](int t, double (&ob)[MAX_OBS]) {             // the block's row of step t, zero-padded as the staged rows of gpf_update_blocks
        const double* const orow = obs_b + (size_t)t * (size_t)a.n_obs;
#pragma unroll
        for (int k = 0; k < MAX_OBS; ++k) ob[k] = k < a.n_obs ? orow[k] : 0.0;
    };
    // ================ prologue: k_init under the twin's epoch 0
    {
        double ob[MAX_OBS];
        obs_row(0, ob);
        for (int j = tl; j < cnt; j += TEAM) {
            double x[MAX_DIM];
            Mo::sample(P, true, nullptr, ob, a.seed, (uint32_t)(a.gid0 + b0 + j), 0, 0u, TAG_INIT, x);
            const double ll = Mo::loglik(P, x, ob);
            double o[W];
#pragma unroll
            for (int k = 0; k < W; ++k) o[k] = 0.0;
#pragma unroll
            for (int k = 0; k < D; ++k) o[k] = x[k];
            double2* dst = reinterpret_cast<double2*>(rbase + (size_t)j * W);
#pragma unroll
            for (int c = 0; c < W / 2; ++c) dst[c] = make_double2(o[2 * c], o[2 * c + 1]);
            lw[j] = ll;
            par[j] = (int32_t)(b0 + j);                            // (k_iota: a block that never resamples keeps the filter-wide identity)
        }
    }
    twin_sync();
    int side = 0;
    double m; int f; uint64_t q[ITEMS]; uint64_t S_w; double ess;
    run_summary<TEAM, ITEMS>(lw, cnt, K, tl, s_m, s_f, s_x, m, f, q, S_w, ess);
    // ================ series: k_block_series<.., RunPlain>'s step for steps 1 .. T-1; the twin's gpf_run_blocks starts at epoch 1
#pragma unroll 1
    for (int t = 1; t < a.n_steps; ++t) {
        const uint32_t ep_r = 1u + 2u * (uint32_t)(t - 1), ep_u = ep_r + 1u;
        const bool gate = a.ess_frac >= 0.0 ? (f == 0 && ess < a.ess_frac * (double)cnt) : true;
        const bool skip = (f & (FLAG_NAN | FLAG_POSINF)) != 0;
        const bool uniform = (f & FLAG_ALL_NEGINF) != 0;
        const bool go = gate && !skip;
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
        double ob[MAX_OBS];
        obs_row(t, ob);
        const double* const rows_in = rbase + (size_t)side * rstride;
        double* const rows_out = rbase + (size_t)(go ? 1 - side : side) * rstride;
        for (int j = tl; j < cnt; j += TEAM) {
            const uint32_t slot = (uint32_t)(a.gid0 + b0 + j);
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
                par[j] = anc;                                      // (block-local, the last write stands: gpf_resample_blocks' parents)
            }
            double r[W];
            {
                const double2* src = reinterpret_cast<const double2*>(rows_in + (size_t)anc * W);
#pragma unroll
                for (int c = 0; c < (D + 1) / 2; ++c) { const double2 v2 = src[c]; r[2 * c] = v2.x; r[2 * c + 1] = v2.y; }
            }
            const double lw_in = go ? new_lw : lw[j];
            double xn[MAX_DIM];
            Mo::sample(P, false, r, ob, a.seed, slot, 0, ep_u, TAG_UPDATE, xn);
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
        if (go) side ^= 1;
        twin_sync();                                               // rows and weights of this step: visible to the team (and s_cdf / s_aux / s_idx free again)
        run_summary<TEAM, ITEMS>(lw, cnt, K, tl, s_m, s_f, s_x, m, f, q, S_w, ess);
    }
    // ================ epilogue: the estimate, the decision, the replacement
    const double logc = log_((double)cnt);
    const double lse_t = lse_from(m, S_w, K, f);
    const double Lp = (0.0 + lse_t) - logc;                        // k_block_stats on the twin: (log_ml_est + logsumexp) - log(cnt), left to right
    bool ok = f == 0 && Lp > a.thr[blk];                           // (strict; the thresholds hold no NaN, a NaN estimate carries a flag)
    double shift = 0.0;
    if (ok && a.keep_mass) {                                       // (team-uniform: the barriers inside the summary are reached by the whole team)
        double ms; int fs; uint64_t qs[ITEMS]; uint64_t Ss; double es;
        run_summary<TEAM, ITEMS>(a.lw + b0, cnt, K, tl, s_m, s_f, s_x, ms, fs, qs, Ss, es);
        ok = fs == 0;
        shift = (lse_from(ms, Ss, K, fs) - logc) - (lse_t - logc); // one double per block: lme_state - lme_twin
    }
    if (tl == 0) { a.acc_out[blk] = ok ? 1 : 0; a.lml_out[blk] = Lp; }
    if (!ok) return;
    {
        const double2* const src = reinterpret_cast<const double2*>(rbase + (size_t)side * rstride);
        double2* const dst = reinterpret_cast<double2*>(a.rows + b0 * W);
        for (int j = tl; j < cnt; j += TEAM) {                     // (slot j's row, weight and parent were written by this lane)
#pragma unroll
            for (int c = 0; c < W / 2; ++c) dst[(size_t)j * (W / 2) + c] = src[(size_t)j * (W / 2) + c];
            a.lw[b0 + j] = a.keep_mass ? lw[j] + shift : lw[j];
            a.anc[b0 + j] = par[j];
        }
    }
    if (tl < MAX_PARAMS) a.blk_params[blk * MAX_PARAMS + tl] = P[tl];
    if (tl < MAX_OBS) a.blk_obs[blk * MAX_OBS + tl] = tl < a.n_obs ? obs_b[(size_t)(a.n_steps - 1) * (size_t)a.n_obs + tl] : 0.0;
}

} // namespace gpf
