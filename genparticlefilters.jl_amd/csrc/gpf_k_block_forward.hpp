// K11d: forward-only smoothing per block  (part of gpf_kernels.hpp; include that header, not this file)
#pragma once

namespace gpf {
// ----------------------------------------------------------------------------- additive smoothing functionals without a store
// gpf_forward_enable_blocks / gpf_block_forward_moments (gpf.h; DESIGN.md 5.8 is the definition; Del Moral, Doucet & Singh 2010, "Forward smoothing using
// sequential Monte Carlo"; Poyiadjis, Doucet & Singh 2011, Biometrika 98): every particle j of the current step carries
//     T^j = [ sum(D) | second, upper triangle | cross(D x D, row = the earlier step) | first(D) | first2, upper triangle ],       F = fwd_F(D) doubles,
// the FFBSm estimate of the additive functional along the paths that end in j.  One pass per step updates it from the previous step's record alone:
//     T_s^j = sum_i q_ij T_{s-1}^i / D_j + (what step s adds),      q_ij = exp_fix(lwa_ij - m_j, K),   lwa_ij = lw_{s-1}[i] + logtrans(P_c, x_{s-1}[i], x_s[j], obs_s[c])
// with gpf_block_smooth's statements for lwa, (m_j, f_j), K, q and D_j (an exact u64 sum), its fallback (f_j != 0: the whole mass on the recorded parent) and
// its lineage check (all parents of block c in ONE block c', else every T of block c is NaN).
// k_block_forward<M> is the TRANSPOSE of k_block_smooth: there the candidates live in lanes and every target costs two team reductions; here the sums over
// i are taken in ASCENDING i with one multiply and one add per term, a lane-private serial loop -- so ONE LANE PER TARGET and the candidates as
// wave-uniform reads (the previous record's row i: D + 1 + F doubles at one address for the whole wave, served by the scalar cache; no LDS, no barrier).
// A wave owns 64 consecutive targets of one block; the waves of a block are independent, so a block of 2048 is the work of 32 waves anywhere on the chip.
// Two passes over the candidates: the maximum with flags, then q, D and the accumulations; logtrans is evaluated twice, no bs x bs array exists.
// A candidate with q_ij == 0 is skipped entirely (0 * x is not +0.0 for every x; a dead candidate may carry a non-finite statistic).
// first != 0 (closing step 1): T = [x | x x' | +0.0 | x | x x'], nothing of the previous record is read.
// The same launch serves the close inside gpf_update_blocks* (out = the other half of the ping-pong, then committed) and the query (the same half as
// scratch, nothing committed).  k_block_forward_reduce is the query's second launch: out[b][f] = tree_j(W^j T^j[f]) with block_norm_weights' W and
// k_block_moments' tree, then last2 = tree_j((W^j x^j[a]) x^j[c]) (pairs_products<true>: gpf_block_smooth_pairs' second at the last step).
constexpr int fwd_F(int d) { return d + d * (d + 1) / 2 + d * d + d + d * (d + 1) / 2; }
struct ForwardArgs {
    const double* rows; int W;                     // the current rows [n][W]: the targets
    const int32_t* map;                            // the step's composed ancestor map g_s, nullptr = no resample in the step
    const double* obs;                             // [nblocks][MAX_OBS] the observation rows the step was entered with, in the current block order
    int64_t n, nb, nblocks;
    int wpb;                                       // waves per block = ceil(nb / WAVE)
    int first;                                     // the step is step 1
};
// the body with the parameter row P (a kernarg array or a row of blk_params: read with constant indices only)
template <int M>
__device__ __forceinline__ void block_forward_wave(const ForwardArgs& a, const double* P, int64_t c, int chunk, const double* __restrict__ px,
                                                   const double* __restrict__ plw, const double* __restrict__ pT, double* __restrict__ Tout)
{
    using Mo = Model<M>;
    constexpr int D = Mo::D, TRI = D * (D + 1) / 2, F = fwd_F(D);
    const int lane = lane_id();
    const int64_t c0 = c * a.nb;
    const int cnt = (int)(a.n - c0 < a.nb ? a.n - c0 : a.nb);
    if (chunk * WAVE >= cnt) return;                               // (wave-uniform: a chunk beyond a short last block)
    const int jl = chunk * WAVE + lane;
    const bool live = jl < cnt;
    const int64_t j = c0 + (live ? jl : 0);                        // (a lane beyond the block computes target 0 and stores nothing)
    double xj[D];
    load_latent<D>(a.rows + j * a.W, xj);
    double* const out = Tout + j * F;
    if (a.first) {                                                 // (kernel-uniform)
        if (live) {
            int t = 0;
#pragma unroll
            for (int r = 0; r < D; ++r) out[t++] = xj[r];
#pragma unroll
            for (int r = 0; r < D; ++r)
#pragma unroll
                for (int s = r; s < D; ++s) out[t++] = xj[r] * xj[s];
#pragma unroll
            for (int r = 0; r < D * D; ++r) out[t++] = 0.0;
#pragma unroll
            for (int r = 0; r < D; ++r) out[t++] = xj[r];
#pragma unroll
            for (int r = 0; r < D; ++r)
#pragma unroll
                for (int s = r; s < D; ++s) out[t++] = xj[r] * xj[s];
        }
        return;
    }
    // ---- the lineage: the block all recorded parents of block c sit in (every wave of the block looks at the whole block)
    int bmin = (int)c, bmax = (int)c;
    if (a.map) {                                                   // (kernel-uniform)
        bmin = 0x7fffffff; bmax = -1;
        for (int i = lane; i < cnt; i += WAVE) {
            const int bl = (int)((uint32_t)a.map[c0 + i] / (uint32_t)a.nb);
            bmin = bl < bmin ? bl : bmin; bmax = bl > bmax ? bl : bmax;
        }
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) { const int u = __shfl_xor(bmin, s, WAVE), v = __shfl_xor(bmax, s, WAVE); bmin = u < bmin ? u : bmin; bmax = v > bmax ? v : bmax; }
    }
    bmin = __builtin_amdgcn_readfirstlane(bmin); bmax = __builtin_amdgcn_readfirstlane(bmax);
    if (bmin != bmax || bmin < 0 || bmin >= a.nblocks) {           // (wave-uniform; a map that leaves the filter is undefined as well, and nothing is read through it)
        if (live) {
#pragma unroll
            for (int t = 0; t < F; ++t) out[t] = __builtin_nan("");
        }
        return;
    }
    const int64_t cp0 = (int64_t)bmin * a.nb;
    const int ccnt = (int)(a.n - cp0 < a.nb ? a.n - cp0 : a.nb);
    const int K = fix_K(ccnt);
    const int pl = (int)((a.map ? (int64_t)a.map[j] : j) - cp0);   // the recorded parent within block c'
    double ob[MAX_OBS];
#pragma unroll
    for (int k = 0; k < MAX_OBS; ++k) ob[k] = a.obs[(size_t)c * MAX_OBS + k];
    const double* __restrict__ cx = px + cp0 * D;                  // the candidates' record: wave-uniform addresses from here on
    const double* __restrict__ clw = plw + cp0;
    const double* __restrict__ cT = pT + cp0 * F;
    // ---- pass 1: the maximum and the flags of lwa over i (team_max_flags' statements)
    double m = -__builtin_huge_val(); int f = 0;
#pragma unroll 1
    for (int i = 0; i < ccnt; ++i) {
        double xi[D];
#pragma unroll
        for (int r = 0; r < D; ++r) xi[r] = cx[(size_t)i * D + r];
        const double v = clw[i] + Mo::logtrans(P, xi, xj, ob);
        if (v != v) f |= FLAG_NAN; else { m = v > m ? v : m; if (v == __builtin_huge_val()) f |= FLAG_POSINF; }
    }
    if (!(f & FLAG_NAN) && m == -__builtin_huge_val()) f |= FLAG_ALL_NEGINF;
    // ---- pass 2: q, D and the sums in ascending i; f != 0: q = 1 for the recorded parent, 0 otherwise
    uint64_t Dj = 0;
    double h[F], xb[D];
#pragma unroll
    for (int t = 0; t < F; ++t) h[t] = 0.0;
#pragma unroll
    for (int r = 0; r < D; ++r) xb[r] = 0.0;
#pragma unroll 1
    for (int i = 0; i < ccnt; ++i) {
        double xi[D];
#pragma unroll
        for (int r = 0; r < D; ++r) xi[r] = cx[(size_t)i * D + r];
        uint64_t q;
        if (f == 0) q = exp_fix(clw[i] + Mo::logtrans(P, xi, xj, ob) - m, K);
        else q = i == pl ? 1ull : 0ull;
        Dj += q;
        if (q != 0) {
            const double qd = (double)q;
            const double* __restrict__ Ti = cT + (size_t)i * F;
#pragma unroll
            for (int t = 0; t < F; ++t) h[t] = h[t] + qd * Ti[t];
#pragma unroll
            for (int r = 0; r < D; ++r) xb[r] = xb[r] + qd * xi[r];
        }
    }
    const double Dd = (double)Dj;
    double xbar[D];
#pragma unroll
    for (int r = 0; r < D; ++r) xbar[r] = xb[r] / Dd;
    if (live) {
        int t = 0;
#pragma unroll
        for (int r = 0; r < D; ++r) { out[t] = h[t] / Dd + xj[r]; ++t; }
#pragma unroll
        for (int r = 0; r < D; ++r)
#pragma unroll
            for (int s = r; s < D; ++s) { out[t] = h[t] / Dd + xj[r] * xj[s]; ++t; }
#pragma unroll
        for (int r = 0; r < D; ++r)
#pragma unroll
            for (int s = 0; s < D; ++s) { out[t] = h[t] / Dd + xbar[r] * xj[s]; ++t; }
#pragma unroll
        for (int r = 0; r < D + TRI; ++r) { out[t] = h[t] / Dd; ++t; }
    }
}
template <int M>
__global__ __launch_bounds__(BLOCK) void k_block_forward(ForwardArgs a, AncArgs x, const double* __restrict__ px, const double* __restrict__ plw,
                                                         const double* __restrict__ pT, double* __restrict__ Tout)
{
    static_assert(Model<M>::D == 1 || Model<M>::D == 2 || Model<M>::D == 4, "the latent columns are moved as words or 16-byte pairs");
    const int64_t gw = (int64_t)blockIdx.x * NWAVES + __builtin_amdgcn_readfirstlane(wave_id());
    if (gw >= a.nblocks * a.wpb) return;                           // (an idle wave: the kernel has no workgroup barrier)
    const int64_t c = gw / a.wpb;
    const int chunk = (int)(gw - c * a.wpb);
    if (x.blk_params) block_forward_wave<M>(a, x.blk_params + c * MAX_PARAMS, c, chunk, px, plw, pT, Tout);   // (kernel-uniform)
    else block_forward_wave<M>(a, x.P, c, chunk, px, plw, pT, Tout);
}
// the query's second launch: out = [nblocks][F + D * D] -- the F weighted trees of T, then last2 [D][D] mirrored; a block with NaN / +Inf weights: NaN
template <int D, int TEAM, int ITEMS>
__global__ __launch_bounds__(BLOCK) void k_block_forward_reduce(const double* __restrict__ T, const double* __restrict__ rows, int W, const double* __restrict__ lw,
                                                                int64_t n, int64_t nb, int64_t nblocks, double* __restrict__ out)
{
    constexpr int TEAMS = BLOCK / TEAM, F = fwd_F(D), ROW = F + D * D;
    static_assert(TEAM == WAVE || TEAM == BLOCK, "a wave or the workgroup");
    __shared__ double s_m[NWAVES];
    __shared__ int s_f[NWAVES];
    __shared__ uint64_t s_x[NWAVES][4];
    __shared__ double s_t[NWAVES][2];
    const int tm = (int)threadIdx.x / TEAM, tl = (int)threadIdx.x % TEAM;
    const int64_t blk = (int64_t)blockIdx.x * TEAMS + tm;
    if (TEAM != BLOCK && blk >= nblocks) return;                   // (an idle wave: the wave-team path has no workgroup barrier)
    const int64_t b0 = blk * nb;
    const int cnt = (int)(n - b0 < nb ? n - b0 : nb);
    double* const o = out + blk * ROW;
    double w[ITEMS];
    const int f = block_norm_weights<TEAM, ITEMS>(lw, b0, cnt, tl, s_m, s_f, s_x, w);
    if (f & (FLAG_NAN | FLAG_POSINF)) {                            // (team-uniform)
        for (int t = tl; t < ROW; t += TEAM) o[t] = __builtin_nan("");
        return;
    }
    const double* __restrict__ Tb = T + b0 * F;
#pragma unroll 1
    for (int t = 0; t < F; t += 2) {
        const bool two = t + 1 < F;
        double t0[ITEMS], t1[ITEMS];
#pragma unroll
        for (int k = 0; k < ITEMS; ++k) {
            const int i = ITEMS * tl + k;
            const bool in = i < cnt;
            t0[k] = in ? w[k] * Tb[(size_t)i * F + t] : 0.0;
            t1[k] = in && two ? w[k] * Tb[(size_t)i * F + t + 1] : 0.0;
        }
        double p[2] = {lane_tree<ITEMS>(t0), lane_tree<ITEMS>(t1)};
        team_tree2<TEAM>(p, s_t);
        if (tl == 0) { o[t] = p[0]; if (two) o[t + 1] = p[1]; }
    }
    double xp[ITEMS][D];
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
        const int i = ITEMS * tl + k;
        if (i < cnt) load_latent<D>(rows + (b0 + i) * W, xp[k]);
        else {
#pragma unroll
            for (int c = 0; c < D; ++c) xp[k][c] = 0.0;
        }
    }
    pairs_products<true, D, TEAM, ITEMS>(w, xp, xp, cnt, tl, s_t, o + F);
}

} // namespace gpf
