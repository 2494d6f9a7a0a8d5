// K11a: ancestor sampling for the conditional block resample  (part of gpf_kernels.hpp; include that header, not this file)
#pragma once

namespace gpf {
// ----------------------------------------------------------------------------- particle Gibbs with ancestor sampling, block by block
// gpf_resample_blocks_ancestor (gpf.h; Lindsten, Jordan & Schoen 2014, "Particle Gibbs with ancestor sampling", JMLR 15): the conditional multinomial
// step of k_block_resample<METHOD_COND> in which the retained particle -- slot 0 of every block that resamples -- draws its ancestor from
//     P(a_0 = i)  proportional to  w_{t-1}^i f(x'_t | x_{t-1}^i),          x'_t = the block's NEXT reference value,
// instead of keeping itself.  Model<M>::logtrans supplies log f up to the terms that do not depend on x_{t-1} (gpf_models.hpp).  Per block:
//   lwa_i = lw_i + logtrans(P_b, x_{t-1}^i, x'_t, obs_b)      the ancestor weights (gpf_block_ancestor_log_weights returns exactly these, k_block_anc_lw)
//   m', flags', q'_i = exp_fix(lwa_i - m', K), S', CDF        the summary every resampler here forms of its weights, in the block's s_cdf
//   a_0 = upper_bound(CDF, mulhi64(U, S'))                    U = resample_u64(seed, gid0 + b0, epoch): slot 0's OWN counter of the call's epoch, the one
//                                                             the unconditional call uses for slot 0 and the conditional call leaves unused
//   flags' hold NaN, +Inf or ALL_NEGINF  ->  a_0 = 0          a reference no particle can lead to keeps its own predecessor: the plain conditional step
// then s_cdf is overwritten with the weight CDF and everything else is METHOD_COND: the slots j >= 1 (same counters, same CDF), the new weights and
// the parents array.  Blocks that do not resample draw no ancestor.  No LDS beyond METHOD_COND's; one more exp_fix pass and scan per block and one
// read of the block's latent columns.  A kernel of its own: BlockArgs and k_block_resample stay as they are.
struct AncArgs {
    double P[MAX_PARAMS];                          // the filter's parameters (kernarg; read with constant indices only)
    const double* blk_params;                      // gpf_set_block_params in force: [block][MAX_PARAMS], else null
    int64_t bp_size;                               // ... the block size of those rows (k_block_anc_lw takes any block size of its own)
    const double* obs;                             // [nblocks][MAX_OBS] the data vectors of the step being entered (zero-padded)
    const double* ref;                             // [nblocks][MAX_DIM] the reference values of that step
};
// host words -> device by a kernel, as k_stage_obs (the copy stays on the compute queue); the caller orders the reuse of `src_host` with an event
static __global__ __launch_bounds__(BLOCK) void k_stage_words(const double* __restrict__ src_host, double* __restrict__ dst, int64_t n_words)
{
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n_words; i += (int64_t)gridDim.x * BLOCK) dst[i] = src_host[i];
}
// the D latent columns of a row
template <int D>
__device__ __forceinline__ void load_latent(const double* __restrict__ row, double (&xp)[D])
{
    if constexpr (D == 1) xp[0] = row[0];
    else {
#pragma unroll
        for (int c = 0; c < D / 2; ++c) { const double2 v = reinterpret_cast<const double2*>(row)[c]; xp[2 * c] = v.x; xp[2 * c + 1] = v.y; }
    }
}
// out[i] = lw[i] + logtrans(P_b, rows[i][0..D), ref_b, obs_b), b = i / nb: the ancestor log-weights of every particle, any block size
template <int M>
__global__ __launch_bounds__(BLOCK) void k_block_anc_lw(AncArgs x, const double* __restrict__ rows, int W, const double* __restrict__ lw, int64_t n, int64_t nb,
                                                        double* __restrict__ out)
{
    using Mo = Model<M>;
    constexpr int D = Mo::D;
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) {
        const size_t b = (uint32_t)i / (uint32_t)nb;             // (n < 2^31 and nb is clamped to n)
        double xp[D], xr[D], ob[MAX_OBS];
        load_latent<D>(rows + i * W, xp);
#pragma unroll
        for (int c = 0; c < D; ++c) xr[c] = x.ref[b * MAX_DIM + c];
#pragma unroll
        for (int c = 0; c < MAX_OBS; ++c) ob[c] = x.obs[b * MAX_OBS + c];
        double lt;
        if (x.blk_params) lt = Mo::logtrans(x.blk_params + (size_t)((uint32_t)i / (uint32_t)x.bp_size) * MAX_PARAMS, xp, xr, ob);   // (grid-uniform)
        else lt = Mo::logtrans(x.P, xp, xr, ob);
        out[i] = lw[i] + lt;
    }
}
// lwa of the lane's ITEMS particles (-Inf beyond the block)
template <int M, int W, int ITEMS>
__device__ __forceinline__ void anc_weights(const double* P, const double* __restrict__ rows_blk, int cnt, int tl, const double* xr, const double* ob,
                                            const double (&lwv)[ITEMS], double (&lwa)[ITEMS])
{
    using Mo = Model<M>;
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
        const int i = ITEMS * tl + k;
        lwa[k] = -__builtin_huge_val();
        if (i < cnt) {
            double xp[Mo::D];
            load_latent<Mo::D>(rows_blk + (size_t)i * W, xp);
            lwa[k] = lwv[k] + Mo::logtrans(P, xp, xr, ob);
        }
    }
}
// teams as in k_block_resample; W = the row width of model M with or without keep_prev
template <int M, int W, int TEAM, int ITEMS>
__global__ __launch_bounds__(BLOCK) void k_block_resample_anc(BlockArgs a, AncArgs x)
{
    constexpr int D = Model<M>::D;
    constexpr int TEAMS = BLOCK / TEAM, CAP = TEAM * ITEMS;        // blocks per workgroup, particles a team holds
    static_assert(TEAM == WAVE || TEAM == BLOCK, "a wave or the workgroup");
    static_assert(W >= D && W % 2 == 0, "rows are copied as 16-byte column pairs");
    __shared__ uint64_t s_cdf_[BLOCK * ITEMS];                     // first the ancestor weights' CDF, then the weights'
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
    // ---- up to the `go` decision: k_block_resample<METHOD_COND>, statement for statement
    double lwv[ITEMS];
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) { const int i = ITEMS * tl + k; lwv[k] = i < cnt ? a.lw[b0 + i] : -__builtin_huge_val(); }
    double m; int f;
    team_max_flags<TEAM, ITEMS>(lwv, tl, cnt, s_m, s_f, m, f);
    uint64_t q[ITEMS];
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) q[k] = ITEMS * tl + k < cnt ? ((f & FLAG_ALL_NEGINF) ? 1ull : exp_fix(lwv[k] - m, K)) : 0ull;
    bool gate = true;                                              // the block passes the ESS test (or there is none)
    if (a.ess_frac >= 0.0) {                                       // (team-uniform)
        unsigned __int128 Q = 0; uint64_t sl = 0;
#pragma unroll
        for (int k = 0; k < ITEMS; ++k) { Q += (unsigned __int128)q[k] * q[k]; sl += q[k]; }
        uint64_t v4[4] = {(uint64_t)Q & 0xffffffffull, (uint64_t)Q >> 32, (uint64_t)(Q >> 64), sl};
        team_sum4<TEAM>(v4, s_x);
        const unsigned __int128 Qt = ((unsigned __int128)v4[2] << 64) + ((unsigned __int128)v4[1] << 32) + v4[0];
        const double ess = ess_from(v4[3], (uint64_t)(Qt >> 64), (uint64_t)Qt);
        gate = f == 0 && ess < a.ess_frac * (double)cnt;
    }
    const bool skip = (f & (FLAG_NAN | FLAG_POSINF)) != 0 || (a.check_true && f != 0);
    const bool go = gate && !skip;
    if (tl == 0) a.resampled[blk] = (go ? 1 : 0) | ((gate ? f : 0) << 8);
    if (!go) {
        // this block keeps its particles: rows move to the other buffer unchanged, weights and parents stay; no ancestor is drawn
        for (int t = tl; t < cnt * (W / 2); t += TEAM)
            reinterpret_cast<double2*>(a.rows_out + b0 * W)[t] = reinterpret_cast<const double2*>(a.rows_in + b0 * W)[t];
        return;
    }
    // ---- the ancestor weights, their maximum, flags and CDF
    double xr[D], ob[MAX_OBS];
#pragma unroll
    for (int c = 0; c < D; ++c) xr[c] = x.ref[blk * MAX_DIM + c];
#pragma unroll
    for (int c = 0; c < MAX_OBS; ++c) ob[c] = x.obs[blk * MAX_OBS + c];
    double lwa[ITEMS];
    if (x.blk_params) anc_weights<M, W, ITEMS>(x.blk_params + blk * MAX_PARAMS, a.rows_in + b0 * W, cnt, tl, xr, ob, lwv, lwa);      // (team-uniform)
    else anc_weights<M, W, ITEMS>(x.P, a.rows_in + b0 * W, cnt, tl, xr, ob, lwv, lwa);
    double m_a; int f_a;
    team_max_flags<TEAM, ITEMS>(lwa, tl, cnt, s_m, s_f, m_a, f_a);
    uint64_t qa[ITEMS];
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) qa[k] = ITEMS * tl + k < cnt ? exp_fix(lwa[k] - m_a, K) : 0ull;
    const uint64_t S_a = team_scan_incl<TEAM, ITEMS>(qa, s_x);
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) s_cdf[ITEMS * tl + k] = qa[k];
    team_sync<TEAM>();
    // every lane evaluates a_0 (a team-uniform search of LDS); invalid ancestor weights: the retained particle keeps itself
    int a0 = 0;
    if (f_a == 0) a0 = lds_upper_bound(s_cdf, cnt, mulhi64(resample_u64(a.seed, (uint32_t)(a.gid0 + b0), a.epoch), S_a));
    team_sync<TEAM>();                                             // (s_cdf is overwritten next)
    // ---- the weight CDF, ancestors, gather, sub-state weights: METHOD_COND with anc = a_0 for slot 0
    const uint64_t S = team_scan_incl<TEAM, ITEMS>(q, s_x);
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) s_cdf[ITEMS * tl + k] = q[k];
    team_sync<TEAM>();
    const double new_lw = lse_from(m, S, K, f) - log_((double)cnt);
    for (int j = tl; j < cnt; j += TEAM) {                         // consecutive lanes, consecutive slots: coalesced stores
        const uint32_t slot = (uint32_t)(a.gid0 + b0 + j);
        int anc = lds_upper_bound(s_cdf, cnt, mulhi64(resample_u64(a.seed, slot, a.epoch), S));
        if (j == 0) anc = a0;
        const double2* src = reinterpret_cast<const double2*>(a.rows_in + (b0 + anc) * W);
        double2* dst = reinterpret_cast<double2*>(a.rows_out + (b0 + j) * W);
#pragma unroll
        for (int c = 0; c < W / 2; ++c) dst[c] = src[c];
        a.anc[b0 + j] = anc;
        a.lw[b0 + j] = new_lw;
    }
}

} // namespace gpf
