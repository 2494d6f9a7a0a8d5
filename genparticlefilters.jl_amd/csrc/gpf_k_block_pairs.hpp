// K11d: pairwise smoothing per block from the trajectory store  (part of gpf_kernels.hpp; include that header, not this file)
#pragma once

namespace gpf {
// ----------------------------------------------------------------------------- the E-step of particle EM, block by block
// gpf_block_smooth_pairs (gpf.h; DESIGN.md 5.7 is the definition): k_block_smooth's walk -- lineage, step-T weights, targets and candidates, lwa_ij,
// (m_j, f_j), K, q_ij, D_j, r_ij, the fallback to the recorded parent, P_b, rounds of NB targets: gpf_k_block_smooth.hpp, whose helpers are used as
// they are -- and beside the smoothing weight of every candidate i of step s the pairwise sums
//     A_i[c] = sum_j t_ij x_{s+1}^j[c],    t_ij = W_{s+1}^j r_ij  (the pairwise smoothing weight of (i, j): the term k_block_smooth adds to W_s^i),
// from +0.0 in ASCENDING j, one multiply and one add per term and column.  A target with W_{s+1}^j == 0 is skipped ENTIRELY (gpf.h): a round with one
// live target still visits its dead ones, so the accumulation of W and A sits under a team-uniform guard -- 0 * x is not +0.0 for every x.  The walk is
// written a second time here, not shared through a template parameter: k_block_smooth's fifteen instantiations stay what they were.
//   state     A is ITEMS x D doubles per lane beside k_block_smooth's registers (xp, lwc, acc, a round's lwa and qv): profiles/block_pairs.md has
//             what the compiler makes of it per instantiation.  A is only accumulated for a pair that is written (cross asked for, s + 1 <= step_hi).
//   second    second_s[a][c] = tree_i((W_s^i x_s^i[a]) x_s^i[c]) for a <= c, mirrored;   cross_s[a][c] = tree_i(x_s^i[a] A_i[c]);   mean as k_block_smooth:
//             k_block_moments' tree (lane_tree, team_tree2) over the index within block c_s, two entries per tree, terms beyond a short block +0.0.
// Outputs (any may be null): mean = [nblocks][n_steps][D], second = [nblocks][n_steps][D][D], cross = [nblocks][n_steps - 1][D][D] (entry o: the pair
// of the 0-based steps lo0 + o and lo0 + o + 1), blocks = [nblocks][n_steps] 1-based c_s.  Steps above hi0 are walked, not written.
struct PairArgs {
    const int32_t* const* maps;                    // as SmoothArgs
    const double* const* hx;
    const double* const* hlw;
    const double* const* hobs;
    const double* lw;
    int T, lo0, hi0;
    int64_t n, nb, nblocks;
    double* mean; double* second; double* cross; int64_t* blocks;
};
// targets per reduction round, by ITEMS (profiles/block_pairs.md); kernel experiments override them (tools/build_variant.sh)
#ifndef GPF_PAIRS_NB2
#define GPF_PAIRS_NB2 2
#endif
#ifndef GPF_PAIRS_NB8
#define GPF_PAIRS_NB8 4
#endif
constexpr int pairs_nb(int items) { return items == 2 ? GPF_PAIRS_NB2 : GPF_PAIRS_NB8; }
static_assert(GPF_PAIRS_NB2 <= SMOOTH_NB_MAX && GPF_PAIRS_NB8 <= SMOOTH_NB_MAX, "the rounds use SmoothLds' words");
// out[a][c] = tree_i(u_i[a] v_i[c]) with u = sc x (SECOND: sc = W, and only a <= c is formed, mirrored) or u = x (cross: v = A), two entries per tree
template <bool SECOND, int D, int TEAM, int ITEMS>
__device__ __forceinline__ void pairs_products(const double (&sc)[ITEMS], const double (&x)[ITEMS][D], const double (&v)[ITEMS][D], int cnt, int tl, double (*s_t)[2],
                                               double* __restrict__ out)
{
#pragma unroll
    for (int a = 0; a < D; ++a) {
#pragma unroll
        for (int c = SECOND ? a : 0; c < D; c += 2) {
            const bool two = c + 1 < D;
            const int c1 = two ? c + 1 : c;
            double t0[ITEMS], t1[ITEMS];
#pragma unroll
            for (int k = 0; k < ITEMS; ++k) {
                const bool in = ITEMS * tl + k < cnt;
                const double u = SECOND ? sc[k] * x[k][a] : x[k][a];
                t0[k] = in ? u * v[k][c] : 0.0;
                t1[k] = in && two ? u * v[k][c1] : 0.0;
            }
            double p[2] = {lane_tree<ITEMS>(t0), lane_tree<ITEMS>(t1)};
            team_tree2<TEAM>(p, s_t);
            if (tl == 0) {
                out[a * D + c] = p[0];
                if (two) out[a * D + c1] = p[1];
                if (SECOND) { out[c * D + a] = p[0]; if (two) out[c1 * D + a] = p[1]; }
            }
        }
    }
}
// the whole walk of final block blk with the parameter row P (block_smooth_walk's, with A beside acc)
template <int M, int TEAM, int ITEMS>
__device__ __forceinline__ void block_pairs_walk(const PairArgs& a, const double* P, int64_t blk, int tl, const SmoothLds& L)
{
    using Mo = Model<M>;
    constexpr int D = Mo::D, NB = pairs_nb(ITEMS);
    const int64_t nb = a.nb;
    const int n_steps = a.hi0 - a.lo0 + 1;
    double* const mean_b = a.mean ? a.mean + blk * n_steps * D : nullptr;
    double* const sec_b = a.second ? a.second + blk * n_steps * (D * D) : nullptr;
    double* const cross_b = a.cross ? a.cross + blk * (n_steps - 1) * (D * D) : nullptr;
    int64_t* const c_b = a.blocks ? a.blocks + blk * n_steps : nullptr;
    // the steps lo0 .. top of this block have no value, and no pair whose lower step is one of them: NaN everywhere, lineage 0
    auto undefined = [&](int top) {
        const int ns = (top < a.hi0 ? top : a.hi0) - a.lo0 + 1;
        const int np = (top < a.hi0 - 1 ? top : a.hi0 - 1) - a.lo0 + 1;
        if (mean_b) for (int t = tl; t < ns * D; t += TEAM) mean_b[t] = __builtin_nan("");
        if (sec_b) for (int t = tl; t < ns * D * D; t += TEAM) sec_b[t] = __builtin_nan("");
        if (cross_b) for (int t = tl; t < np * D * D; t += TEAM) cross_b[t] = __builtin_nan("");
        if (c_b) for (int t = tl; t < ns; t += TEAM) c_b[t] = 0;
    };
    int64_t c = blk, c0 = c * nb;
    int cnt = (int)(a.n - c0 < nb ? a.n - c0 : nb);
    // ---- step T: the block's current normalised weights
    double w[ITEMS];
    const int f = block_norm_weights<TEAM, ITEMS>(a.lw, c0, cnt, tl, L.s_m, L.s_f, L.s_x, w);
    if (f & (FLAG_NAN | FLAG_POSINF)) { undefined(a.T - 1); return; }   // (team-uniform)
    double xp[ITEMS][D];
    smooth_load_rows<D, ITEMS>(a.hx[a.T - 1] + c0 * D, cnt, tl, xp);
    for (int q = a.T - 1; ; --q) {
        // ---- what step q returns: xp and w are block c's rows and smoothing weights of that step
        if (q <= a.hi0) {
            const int o = q - a.lo0;
            if (mean_b) smooth_moments<D, TEAM, ITEMS>(w, xp, cnt, tl, L.s_t, mean_b + o * D, nullptr);
            if (sec_b) pairs_products<true, D, TEAM, ITEMS>(w, xp, xp, cnt, tl, L.s_t, sec_b + o * (D * D));
            if (c_b && tl == 0) c_b[o] = c + 1;
        }
        if (q == a.lo0) break;
        // ---- the lineage: the block all recorded parents of block c sit in
        const int32_t* __restrict__ g = a.maps[q];                 // (kernel-uniform)
        int bmin = 0x7fffffff, bmax = -1;
#pragma unroll
        for (int k = 0; k < ITEMS; ++k) {
            const int i = ITEMS * tl + k;
            if (i < cnt) {
                const int64_t pm = g ? (int64_t)g[c0 + i] : c0 + i;
                const int bl = (int)((uint32_t)pm / (uint32_t)nb);
                bmin = bl < bmin ? bl : bmin; bmax = bl > bmax ? bl : bmax;
            }
        }
        smooth_min_max<TEAM>(bmin, bmax, L.s_c);
        if (bmin != bmax) { undefined(q - 1); return; }            // (team-uniform)
        // ---- W of the targets to LDS; the candidates of step q - 1 to registers
        team_sync<TEAM>();                                         // (the previous step's rounds have read L.W)
#pragma unroll
        for (int k = 0; k < ITEMS; ++k) L.W[ITEMS * tl + k] = w[k];
        team_sync<TEAM>();
        const int64_t cp = bmin, cp0 = cp * nb;
        const int ccnt = (int)(a.n - cp0 < nb ? a.n - cp0 : nb);
        const int K = fix_K(ccnt);
        smooth_load_rows<D, ITEMS>(a.hx[q - 1] + cp0 * D, ccnt, tl, xp);
        const double* __restrict__ plw = a.hlw[q - 1] + cp0;
        double lwc[ITEMS], acc[ITEMS], A[ITEMS][D];
#pragma unroll
        for (int k = 0; k < ITEMS; ++k) {
            const int i = ITEMS * tl + k;
            lwc[k] = i < ccnt ? plw[i] : -__builtin_huge_val(); acc[k] = 0.0;
#pragma unroll
            for (int cc = 0; cc < D; ++cc) A[k][cc] = 0.0;
        }
        const bool pair = cross_b && q <= a.hi0;                   // (kernel-uniform: the pair (q - 1, q) is written)
        double ob[MAX_OBS];
        const double* __restrict__ orow = a.hobs[q] + (size_t)c * MAX_OBS;
#pragma unroll
        for (int k = 0; k < MAX_OBS; ++k) ob[k] = orow[k];
        const double* __restrict__ xt = a.hx[q] + c0 * D;          // the targets' rows: one broadcast address each
#pragma unroll 1
        for (int j0 = 0; j0 < cnt; j0 += NB) {
            double Wj[NB]; bool any = false;
#pragma unroll
            for (int t = 0; t < NB; ++t) { Wj[t] = j0 + t < cnt ? L.W[j0 + t] : 0.0; any = any || Wj[t] != 0.0; }
            if (!any) continue;                                    // (team-uniform)
            double lwa[NB][ITEMS], xr[NB][D];
#pragma unroll
            for (int t = 0; t < NB; ++t) {
                const int j = j0 + t < cnt ? j0 + t : j0;          // (beyond the block: W = 0, any row)
                load_latent<D>(xt + (size_t)j * D, xr[t]);
#pragma unroll
                for (int k = 0; k < ITEMS; ++k) {
                    lwa[t][k] = -__builtin_huge_val();
                    if (ITEMS * tl + k < ccnt) lwa[t][k] = lwc[k] + Mo::logtrans(P, xp[k], xr[t], ob);
                }
            }
            double mj[NB]; int fj[NB];
            smooth_max_flags<TEAM, ITEMS, NB>(lwa, tl, ccnt, L.rm, L.rf, mj, fj);
            uint64_t qv[NB][ITEMS], Dj[NB];
#pragma unroll
            for (int t = 0; t < NB; ++t) {
                Dj[t] = 0;
#pragma unroll
                for (int k = 0; k < ITEMS; ++k) { qv[t][k] = ITEMS * tl + k < ccnt ? exp_fix(lwa[t][k] - mj[t], K) : 0ull; Dj[t] += qv[t][k]; }
            }
            smooth_sum<TEAM, NB>(Dj, L.rd);
#pragma unroll
            for (int t = 0; t < NB; ++t) {                         // ascending j
                if (Wj[t] != 0.0) {                                // (team-uniform: a dead target of a live round is skipped entirely)
                    const double Dd = (double)Dj[t];
                    // invalid ancestor weights (f_j != 0, team-uniform): the whole mass of the target goes to its recorded parent
                    const int j = j0 + t;
                    const int pl = fj[t] == 0 ? -1 : (int)((g ? (int64_t)g[c0 + j] : c0 + j) - cp0);
#pragma unroll
                    for (int k = 0; k < ITEMS; ++k) {
                        const double r = fj[t] == 0 ? (double)qv[t][k] / Dd : (ITEMS * tl + k == pl ? 1.0 : 0.0);
                        const double term = Wj[t] * r;
                        acc[k] = acc[k] + term;
                        if (pair) {
#pragma unroll
                            for (int cc = 0; cc < D; ++cc) A[k][cc] = A[k][cc] + term * xr[t][cc];
                        }
                    }
                }
            }
        }
        if (pair) pairs_products<false, D, TEAM, ITEMS>(acc, xp, A, ccnt, tl, L.s_t, cross_b + (q - 1 - a.lo0) * (D * D));
#pragma unroll
        for (int k = 0; k < ITEMS; ++k) w[k] = acc[k];
        c = cp; c0 = cp0; cnt = ccnt;
    }
}
template <int M, int TEAM, int ITEMS>
__global__ __launch_bounds__(BLOCK) void k_block_smooth_pairs(PairArgs a, AncArgs x)
{
    constexpr int TEAMS = BLOCK / TEAM, CAP = TEAM * ITEMS;
    static_assert(TEAM == WAVE || TEAM == BLOCK, "a wave or the workgroup");
    static_assert(Model<M>::D == 1 || Model<M>::D == 2 || Model<M>::D == 4, "the latent columns are moved as words or 16-byte pairs");
    __shared__ double s_W_[BLOCK * ITEMS];
    __shared__ double s_rm[NWAVES][SMOOTH_NB_MAX];
    __shared__ int s_rf[NWAVES][SMOOTH_NB_MAX];
    __shared__ uint64_t s_rd[NWAVES][SMOOTH_NB_MAX];
    __shared__ double s_m[NWAVES];
    __shared__ int s_f[NWAVES];
    __shared__ uint64_t s_x[NWAVES][4];
    __shared__ double s_t[NWAVES][2];
    __shared__ int s_c[NWAVES][2];
    const int tm = (int)threadIdx.x / TEAM, tl = (int)threadIdx.x % TEAM;
    const int64_t blk = (int64_t)blockIdx.x * TEAMS + tm;
    if (TEAM != BLOCK && blk >= a.nblocks) return;                 // (an idle wave: the wave-team path has no workgroup barrier)
    const SmoothLds L{s_W_ + tm * CAP, s_rm, s_rf, s_rd, s_m, s_f, s_x, s_t, s_c};
    if (x.blk_params) block_pairs_walk<M, TEAM, ITEMS>(a, x.blk_params + blk * MAX_PARAMS, blk, tl, L);     // (team-uniform)
    else block_pairs_walk<M, TEAM, ITEMS>(a, x.P, blk, tl, L);
}

} // namespace gpf
