// K11f: a whole series per block in one launch  (part of gpf_kernels.hpp; include that header, not this file)
#pragma once

namespace gpf {
// ----------------------------------------------------------------------------- the filter loop of many small filters, block by block
// gpf_run_blocks (gpf.h): the README loop of test/resample.jl:130-162 per block,
//     for t in 1:T;  pf_resample_blocks(state, bs, method, ess_frac, check = false);  pf_update_blocks(state, ..., ys[:, t], bs);  end
// in ONE launch.  The blocks never interact inside that loop and a block of <= 2048 particles is the work of one team (team_dispatch), so team b
// runs all n_steps iterations of block b with nothing but team barriers between them.  Per step, statement for statement:
//   resample   the body of k_block_resample<METHOD> (non-PRIO, non-COND, check = false) under epoch E + 2t: the ESS gate, the optional bitonic
//              order, the CDF(s) in LDS, the search of slot gid0 + b0 + j.  The weight summary it opens with is the one the previous step closed with
//              (below); the row gather feeds the propagate directly instead of going through memory;
//   propagate  the default-proposal body of k_step<M, W, false, false, 0, false, true> for the block's slots under epoch E + 2t + 1, TAG_UPDATE, RNG
//              counter gid0 + b0 + j: Model<M>::sample from the (gathered) row, loglik, lw = (new weight | lw) + ll;
//   summary    the body of k_block_stats over the new weights: maximum, flags, fixed-point weights, their sum and sum of squares.  It is step t's
//              ess_out / lml_out AND the gate and the weights of step t + 1's resample: both kernels form (m, f) by the same statements in the same
//              order (per lane ascending k, the wave's butterfly, the waves ascending) and everything after them is exact integer arithmetic
//              (exp_fix of the same argument, u64 / u128 sums), so the values are the same bits; formed once.
// Rows: a block that resamples reads its ancestors' rows in one row buffer and writes the propagated rows into the other; a block that does not
// propagates in place.  `side` says which buffer holds the block's rows; after the last step a block that ended in the other buffer copies its rows
// back, so that every block's rows sit in rows[0] -- the handle's current buffer, where the loop leaves them (two flips per iteration).
// Parameters: block b's row of blk_params where per-block parameters are set, else the filter's (a device copy: one pointer, team-uniform).
// Observations: obs[b | 0][t][n_obs], the caller's own layout (a transposition to step-major on the host cost more than the launch: profiles/block_run.md),
// read by (b, t) and zero-padded to MAX_OBS in registers; obs_blocks == 1: one series for all blocks.
// Synchronisation: rows and log-weights written by one lane are read by other lanes of the team in the next phase, through GLOBAL memory.  team_sync
// does not promise that for the wave team: its wavefront-scope fences are compiler barriers only.  run_sync is a release / acquire pair at WORKGROUP
// scope around the team's barrier -- for the workgroup team that is __syncthreads, for the wave team the same two fences around the wave barrier.
// What hipcc makes of them on gfx950 (read in the unit's ISA): s_waitcnt lgkmcnt(0) in front of the barrier and no cache instruction -- a workgroup's
// waves share their CU's L1, which serves the vector memory operations of the CU in issue order, so a load issued behind the barrier is behind the
// store issued in front of it; that is the guarantee every store -> __syncthreads -> load through global memory in a HIP program rests on.  No spin
// waits, nothing between workgroups; every loop is bounded by n_steps, cnt or the network's size.
struct RunArgs {
    double* rows[2];                               // [n][W]; rows[0] holds the rows on entry and on exit
    double* lw;                                    // [n]
    int32_t* anc;                                  // [n] parents, local to the block, written by the blocks that resample (last write wins)
    int64_t n, nb, nblocks, gid0;
    uint64_t seed; uint32_t epoch;                 // E: the resample of step t runs under E + 2t, the propagate under E + 2t + 1
    int32_t n_steps;
    int sorted;                                    // stratified: sort_particles
    double ess_frac;                               // < 0: every block resamples at every step
    const double* P;                               // [MAX_PARAMS] the filter's parameters (device)
    const double* blk_params;                      // [nblocks][MAX_PARAMS] or null
    const double* obs; int64_t obs_blocks;         // [obs_blocks][n_steps][n_obs], the caller's layout; obs_blocks = nblocks | 1
    int32_t n_obs;                                 // the model's, 1 .. MAX_OBS
    const double* lml_est;
    double* ess_out; double* lml_out;              // [n_steps][nblocks]: k_block_stats after step t's update
    int32_t* res_out;                              // [n_steps][nblocks]: the word k_block_resample leaves in blk_mask at step t
    int32_t* flags_out;                            // [nblocks]: (OR of the block's validity flags over the steps) << 8 (k_block_summary folds them)
    double* blk_obs;                               // [nblocks][MAX_OBS] the handle's per-block observation rows: the last step's
};
template <int TEAM>
__device__ __forceinline__ void run_sync()
{
    if (TEAM == BLOCK) __syncthreads();
    else { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup"); }
}
// what a step closes and the next one opens with: maximum, flags, fixed-point weights, their sum and the ESS of the block's current log-weights
template <int TEAM, int ITEMS>
__device__ __forceinline__ void run_summary(const double* lw_blk, int cnt, int K, int tl, double* s_m, int* s_f, uint64_t (*s_x)[4],
                                            double& m, int& f, uint64_t (&q)[ITEMS], uint64_t& S, double& ess)
{
    double lwv[ITEMS];
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) { const int i = ITEMS * tl + k; lwv[k] = i < cnt ? lw_blk[i] : -__builtin_huge_val(); }
    team_max_flags<TEAM, ITEMS>(lwv, tl, cnt, s_m, s_f, m, f);
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) q[k] = ITEMS * tl + k < cnt ? ((f & FLAG_ALL_NEGINF) ? 1ull : exp_fix(lwv[k] - m, K)) : 0ull;
    unsigned __int128 Q = 0; uint64_t sl = 0;
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) { Q += (unsigned __int128)q[k] * q[k]; sl += q[k]; }
    uint64_t v4[4] = {(uint64_t)Q & 0xffffffffull, (uint64_t)Q >> 32, (uint64_t)(Q >> 64), sl};
    team_sum4<TEAM>(v4, s_x);
    S = v4[3];
    const unsigned __int128 Qt = ((unsigned __int128)v4[2] << 64) + ((unsigned __int128)v4[1] << 32) + v4[0];
    ess = ess_from(S, (uint64_t)(Qt >> 64), (uint64_t)Qt);
}
template <int M, int W, int METHOD, int TEAM, int ITEMS>    // METHOD 0 multinomial, 1 residual, 2 stratified; W = row_width(Model<M>::D, false)
__global__ __launch_bounds__(BLOCK) void k_block_run(RunArgs a)
{
    using Mo = Model<M>;
    constexpr int D = Mo::D;
    constexpr int TEAMS = BLOCK / TEAM, CAP = TEAM * ITEMS;        // blocks per workgroup, particles a team holds
    static_assert(TEAM == WAVE || TEAM == BLOCK, "a wave or the workgroup");
    static_assert(W >= D && W % 2 == 0, "rows are moved as 16-byte column pairs");
    __shared__ uint64_t s_cdf_[BLOCK * ITEMS];                     // the CDF that is sampled (weights; residual: residual weights)
    __shared__ uint64_t s_aux_[METHOD == 0 ? 1 : BLOCK * ITEMS];   // residual: copy-count CDF; stratified: sort keys
    __shared__ uint16_t s_idx_[METHOD == 2 ? BLOCK * ITEMS : 1];   // stratified, sorted: the order
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
    const int cnt = (int)(a.n - b0 < a.nb ? a.n - b0 : a.nb);      // particles of this block
    const int K = fix_K(cnt);
    const double* const P = a.blk_params ? a.blk_params + blk * MAX_PARAMS : a.P;      // (team-uniform)
    const double* const obs_b = a.obs + (a.obs_blocks == 1 ? 0 : (size_t)blk * (size_t)a.n_steps * (size_t)a.n_obs);      // the block's series
    const double lml0 = *a.lml_est;
    double* const lw = a.lw + b0;
    int side = 0, flags_all = 0;
    double m; int f; uint64_t q[ITEMS]; uint64_t S_w; double ess;
    run_summary<TEAM, ITEMS>(lw, cnt, K, tl, s_m, s_f, s_x, m, f, q, S_w, ess);
#pragma unroll 1
    for (int t = 0; t < a.n_steps; ++t) {
        // ================ k_block_resample<METHOD>, epoch E + 2t
        const uint32_t ep_r = a.epoch + 2u * (uint32_t)t, ep_u = ep_r + 1u;
        // `effective_sample_size(state) < N / 2`, README.md:72; invalid weights: the reference's ESS is NaN and the comparison false
        const bool gate = a.ess_frac >= 0.0 ? (f == 0 && ess < a.ess_frac * (double)cnt) : true;
        const bool skip = (f & (FLAG_NAN | FLAG_POSINF)) != 0;     // NaN / +Inf: Categorical rejects them in the reference -- left as it stands
        const bool uniform = (f & FLAG_ALL_NEGINF) != 0;
        const bool go = gate && !skip;
        if (tl == 0) a.res_out[(int64_t)t * a.nblocks + blk] = (go ? 1 : 0) | ((gate ? f : 0) << 8);
        flags_all |= gate ? f : 0;
        uint64_t S = 0, Ctot = 0, Rs = 0;
        if (go) {
            // ---- sort_particles (stratified, resample.jl:156-157): the bitonic network over (key, index) pairs
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
            // ---- the CDF(s)
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
        // (resample.jl:205-211: every particle of a block that resampled carries the block's average weight)
        const double new_lw = go ? lse_from(m, S, K, f) - log_((double)cnt) : 0.0;
        const uint64_t sB = METHOD == 2 && go ? S / (uint64_t)cnt : 0, srem = METHOD == 2 && go ? S % (uint64_t)cnt : 0;
        // ================ the slots: ancestor (resample), then k_step's default proposal under epoch E + 2t + 1
        double ob[MAX_OBS];                                        // (team-uniform: the block's row of step t, zero-padded as the staged rows of gpf_update_blocks)
        {
            const double* const orow = obs_b + (size_t)t * (size_t)a.n_obs;
#pragma unroll
            for (int k = 0; k < MAX_OBS; ++k) ob[k] = k < a.n_obs ? orow[k] : 0.0;
        }
        const double* const rows_in = a.rows[side] + b0 * W;
        double* const rows_out = a.rows[go ? 1 - side : side] + b0 * W;
        for (int j = tl; j < cnt; j += TEAM) {                     // consecutive lanes, consecutive slots: coalesced stores
            const uint32_t slot = (uint32_t)(a.gid0 + b0 + j);
            int anc = j;
            if (go) {
                if (METHOD == 0) anc = lds_upper_bound(s_cdf, cnt, mulhi64(resample_u64(a.seed, slot, ep_r), S));          // :59
                else if (METHOD == 1) {
                    if ((uint64_t)j < Ctot) anc = lds_upper_bound(s_aux, cnt, (uint64_t)j);                                 // :101 (no draw)
                    else anc = lds_upper_bound(s_cdf, cnt, mulhi64(resample_u64(a.seed, slot, ep_r), Rs));                  // :113
                } else {
                    const uint64_t jl = (uint64_t)j;                                                               // strata are local to the block
                    const uint64_t L0 = jl * sB + (uint32_t)(jl * srem) / (uint32_t)cnt, L1 = (jl + 1) * sB + (uint32_t)((jl + 1) * srem) / (uint32_t)cnt;
                    anc = lds_upper_bound(s_cdf, cnt, L0 + mulhi64(resample_u64(a.seed, slot, ep_r), L1 - L0));           // :162-166
                    if (a.sorted) anc = (int)s_idx[anc];                                                           // :168
                }
                a.anc[b0 + j] = anc;
            }
            double r[W];
            {
                const double2* src = reinterpret_cast<const double2*>(rows_in + (size_t)anc * W);
#pragma unroll
                for (int c = 0; c < (D + 1) / 2; ++c) { const double2 v = src[c]; r[2 * c] = v.x; r[2 * c + 1] = v.y; }
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
        run_sync<TEAM>();                                          // rows and weights of this step: visible to the team (and s_cdf / s_aux / s_idx free again)
        // ================ k_block_stats: step t's outputs, step t + 1's gate and weights
        run_summary<TEAM, ITEMS>(lw, cnt, K, tl, s_m, s_f, s_x, m, f, q, S_w, ess);
        if (tl == 0) {
            a.ess_out[(int64_t)t * a.nblocks + blk] = f ? __builtin_nan("") : ess;                          // (lognorm of invalid weights is NaN)
            a.lml_out[(int64_t)t * a.nblocks + blk] = (lml0 + lse_from(m, S_w, K, f)) - log_((double)cnt);  // utils.jl:174-178, left to right
        }
    }
    if (tl == 0) a.flags_out[blk] = flags_all << 8;
    if (tl < MAX_OBS)                                              // the block's row of the handle's per-block observations: the last step's
        a.blk_obs[blk * MAX_OBS + tl] = tl < a.n_obs ? obs_b[(size_t)(a.n_steps - 1) * (size_t)a.n_obs + tl] : 0.0;
    if (side)                                                      // (the last step's run_sync ordered the rows)
        for (int e = tl; e < cnt * (W / 2); e += TEAM)
            reinterpret_cast<double2*>(a.rows[0] + b0 * W)[e] = reinterpret_cast<const double2*>(a.rows[1] + b0 * W)[e];
}

} // namespace gpf
