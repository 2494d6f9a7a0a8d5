// K11c: marginal and pairwise smoothing per block from the trajectory store  (part of gpf_kernels.hpp; include that header, not this file)
#pragma once
#include <type_traits>

namespace gpf {
// ----------------------------------------------------------------------------- forward filtering, backward smoothing, block by block
// gpf_block_smooth (gpf.h; FFBSm: Hürzeler & Künsch 1998, "Monte Carlo approximations for general state-space models", JCGS 7; Doucet, Godsill &
// Andrieu 2000, "On sequential Monte Carlo sampling methods for Bayesian filtering", Stat. Comput. 10): deterministic smoothing weights for every
// particle of every recorded step,
//     W_T^j = w_T^j,        W_s^i = sum_j  W_{s+1}^j  w_s^i f(x_{s+1}^j | x_s^i) / sum_l w_s^l f(x_{s+1}^j | x_s^l),
// and the smoothed mean and variance of every latent column under them.  Nothing is drawn.  ONE launch for all blocks and steps; one team per FINAL
// block b, steps outer, targets inner (0-based step q below = step s = q + 1 of gpf.h; DESIGN.md 5.6 is the definition).  The walk is
// block_store_walk, ONE text for k_block_smooth and k_block_smooth_pairs (the E-step of particle EM, below):
//   lineage   c_T = b; c_s = g_{s+1}[c_{s+1} bs] / bs, the block the lineage occupied at step s (b itself unless a resample across blocks moved it).  The
//             team checks that ALL particles of block c_{s+1} have their recorded parent in one block (a team-uniform min / max of pm / bs); where they do
//             not -- a whole-filter resample inside a block-wise step -- the lineage is undefined: from that step down block b reads NaN (lineage 0).
//   step T    W = (double)q_j / (double)S of block_norm_weights: the block's current normalised weights; NaN / +Inf weights: everything of block b NaN.
//   step s    targets j: the particles of block c_{s+1} in snapshot s + 1; candidates i: the particles of block c_s in snapshot s, ITEMS per lane -- their
//             latent columns, recorded log-weight and accumulator stay in the lane's registers for the whole step.  For each target, k_block_backward's
//             statements: lwa_ij = hist_lw[s][i] + logtrans(P_b, hist_x[s][i], hist_x[s+1][j], hist_obs[s+1][c_{s+1}]) (the statement of anc_weights on
//             the register copy of the row), (m_j, f_j) maximum and flags over i, K = fix_K(count of c_s), q_ij = exp_fix(lwa_ij - m_j, K), D_j = sum_i
//             q_ij (u64, exact: any order gives the same bits), r_ij = (double)q_ij / (double)D_j; f_j != 0 (NaN, +Inf, all -Inf): r_ij = 1 for the
//             recorded parent of j and 0 otherwise.  W_s^i = sum_j W_{s+1}^j r_ij from +0.0 in ASCENDING j, one multiply and one add per term (the
//             library is built with contraction off), not renormalised.
//   rounds    NB = smooth_nb(ITEMS) / pairs_nb(ITEMS) targets per reduction round: the target's columns, its W (staged in LDS: <= 16 KB at 2048) and the
//             observation row are team-uniform addresses; the two reductions of a round (maximum with flags, u64 sum) carry NB targets each, so the
//             shuffle chains of a wave team overlap and the workgroup team pays two barriers per round, not four per target.  A lane still adds in
//             ascending j.  A round whose targets all have W = 0 is skipped (adding +0.0 changes no bit); a target beyond the block has W = 0.
//   moments   mean = tree(W_s^i x_s^i), var = tree(W_s^i (x_s^i - mean)^2) with k_block_moments' tree (lane_tree, team_tree2) over the index within the
//             block, for all D latent columns: at s = T this is gpf_block_moments bit for bit.
// P_b: the FINAL block's row of blk_params where per-block parameters are set, else the filter's (as k_block_backward).
// gpf_block_smooth_pairs (gpf.h; DESIGN.md 5.7 is the definition) adds, beside the smoothing weight of every candidate i of step s, the pairwise sums
//     A_i[c] = sum_j t_ij x_{s+1}^j[c],    t_ij = W_{s+1}^j r_ij  (the pairwise smoothing weight of (i, j): the term the walk adds to W_s^i),
// from +0.0 in ASCENDING j, one multiply and one add per term and column.  The statements only its instantiation has (if constexpr (PAIRS)):
//   skip      a target with W_{s+1}^j == 0 is skipped ENTIRELY (gpf.h): a round with one live target still visits its dead ones, so the accumulation of
//             W and A sits under a team-uniform guard -- 0 * x is not +0.0 for every x.  (For W alone the guard changes no bit; k_block_smooth has none.)
//   state     A is ITEMS x D doubles per lane beside the walk's registers (xp, lwc, acc, a round's lwa and qv), and a round's NB target rows stay alive
//             for the accumulation (k_block_smooth holds one row at a time): profiles/block_pairs.md has what the compiler makes of it per
//             instantiation.  A is only accumulated for a pair that is written (cross asked for, s + 1 <= step_hi).
//   second    second_s[a][c] = tree_i((W_s^i x_s^i[a]) x_s^i[c]) for a <= c, mirrored;   cross_s[a][c] = tree_i(x_s^i[a] A_i[c]);   the same tree, two
//             entries per tree, terms beyond a short block +0.0.  No var, no weight rows.
// Outputs (any may be null), n_steps = hi0 - lo0 + 1: mean = [nblocks][n_steps][D], blocks = [nblocks][n_steps] 1-based c_s; k_block_smooth: var as mean,
// wout = [nblocks][n_steps][nb] (0 beyond a short block); k_block_smooth_pairs: second = [nblocks][n_steps][D][D], cross = [nblocks][n_steps - 1][D][D]
// (entry o: the pair of the 0-based steps lo0 + o and lo0 + o + 1).  Steps above hi0 are walked, not written.
struct StoreWalkArgs {                             // what the walk reads
    const int32_t* const* maps;                    // [T] composed ancestor maps, nullptr = no resample in that step
    const double* const* hx;                       // [T] snapshots [n][D]
    const double* const* hlw;                      // [T] recorded log-weights [n]
    const double* const* hobs;                     // [T] recorded observation rows [nblocks][MAX_OBS]
    const double* lw;                              // the current log-weights
    int T, lo0, hi0;
    int64_t n, nb, nblocks;
};
struct SmoothArgs : StoreWalkArgs { double* mean; double* var; double* wout; int64_t* blocks; };
struct PairArgs : StoreWalkArgs { double* mean; double* second; double* cross; int64_t* blocks; };
// targets per reduction round, by ITEMS: 2 on the 2-per-lane wave team (more cost occupancy), 4 on the 8-per-lane teams (within 5 % of 1 and 2) --
// measured, profiles/block_smooth.md and profiles/block_pairs.md; kernel experiments override them (tools/build_variant.sh)
#ifndef GPF_SMOOTH_NB2
#define GPF_SMOOTH_NB2 2
#endif
#ifndef GPF_SMOOTH_NB8
#define GPF_SMOOTH_NB8 4
#endif
#ifndef GPF_PAIRS_NB2
#define GPF_PAIRS_NB2 2
#endif
#ifndef GPF_PAIRS_NB8
#define GPF_PAIRS_NB8 4
#endif
constexpr int SMOOTH_NB_MAX = GPF_SMOOTH_NB2 > GPF_SMOOTH_NB8 ? GPF_SMOOTH_NB2 : GPF_SMOOTH_NB8;
constexpr int smooth_nb(int items) { return items == 2 ? GPF_SMOOTH_NB2 : GPF_SMOOTH_NB8; }
constexpr int pairs_nb(int items) { return items == 2 ? GPF_PAIRS_NB2 : GPF_PAIRS_NB8; }
static_assert(GPF_PAIRS_NB2 <= SMOOTH_NB_MAX && GPF_PAIRS_NB8 <= SMOOTH_NB_MAX, "the rounds use SmoothLds' words");
struct SmoothLds {
    double* W;                                     // [CAP] the smoothing weights of the targets' step
    double (*rm)[SMOOTH_NB_MAX]; int (*rf)[SMOOTH_NB_MAX]; uint64_t (*rd)[SMOOTH_NB_MAX];      // [NWAVES] a round's partial maxima, flags and sums (TEAM = BLOCK only)
    double* s_m; int* s_f; uint64_t (*s_x)[4]; double (*s_t)[2]; int (*s_c)[2];    // block_norm_weights', team_tree2's and the lineage check's words
};
// team_max_flags for NB value sets at once: the same statements per set.  No leading barrier: a wave writes rm / rf of the next round only after the
// barrier of smooth_sum, which every wave reaches after it has read this round's
template <int TEAM, int ITEMS, int NB>
__device__ __forceinline__ void smooth_max_flags(const double (&v)[NB][ITEMS], int tl, int cnt, double (*rm)[SMOOTH_NB_MAX], int (*rf)[SMOOTH_NB_MAX], double (&m_out)[NB], int (&f_out)[NB])
{
#pragma unroll
    for (int t = 0; t < NB; ++t) {
        double m = -__builtin_huge_val(); int f = 0;
#pragma unroll
        for (int k = 0; k < ITEMS; ++k)
            if (ITEMS * tl + k < cnt) { const double x = v[t][k]; if (x != x) f |= FLAG_NAN; else { m = x > m ? x : m; if (x == __builtin_huge_val()) f |= FLAG_POSINF; } }
        m = wave_max_f64(m);
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) f |= __shfl_xor(f, s, WAVE);
        m_out[t] = m; f_out[t] = f;
    }
    if (TEAM == BLOCK) {
        if (lane_id() == 0) {
#pragma unroll
            for (int t = 0; t < NB; ++t) { rm[wave_id()][t] = m_out[t]; rf[wave_id()][t] = f_out[t]; }
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < NB; ++t) {
#pragma unroll
            for (int w = 0; w < NWAVES; ++w) { m_out[t] = rm[w][t] > m_out[t] ? rm[w][t] : m_out[t]; f_out[t] |= rf[w][t]; }
        }
    }
#pragma unroll
    for (int t = 0; t < NB; ++t) if (!(f_out[t] & FLAG_NAN) && m_out[t] == -__builtin_huge_val()) f_out[t] |= FLAG_ALL_NEGINF;
}
// NB exact sums over the team (rd of the next round is written after the barrier of smooth_max_flags: every wave has read this round's by then)
template <int TEAM, int NB>
__device__ __forceinline__ void smooth_sum(uint64_t (&d)[NB], uint64_t (*rd)[SMOOTH_NB_MAX])
{
#pragma unroll
    for (int t = 0; t < NB; ++t) d[t] = wave_sum_u64(d[t]);
    if (TEAM == BLOCK) {
        if (lane_id() == 0) {
#pragma unroll
            for (int t = 0; t < NB; ++t) rd[wave_id()][t] = d[t];
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < NB; ++t) { uint64_t s = 0; for (int w = 0; w < NWAVES; ++w) s += rd[w][t]; d[t] = s; }
    }
}
// minimum and maximum of an int over the team (every thread gets both)
template <int TEAM>
__device__ __forceinline__ void smooth_min_max(int& lo, int& hi, int (*s_c)[2])
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) { const int a = __shfl_xor(lo, s, WAVE), b = __shfl_xor(hi, s, WAVE); lo = a < lo ? a : lo; hi = b > hi ? b : hi; }
    if (TEAM == BLOCK) {
        __syncthreads();                                           // (s_c may still be read from the previous step)
        if (lane_id() == 0) { s_c[wave_id()][0] = lo; s_c[wave_id()][1] = hi; }
        __syncthreads();
#pragma unroll
        for (int w = 0; w < NWAVES; ++w) { lo = s_c[w][0] < lo ? s_c[w][0] : lo; hi = s_c[w][1] > hi ? s_c[w][1] : hi; }
    }
}
// mean and var of the D columns held in registers under the weights w: k_block_hist_moments' statements.  mean_o may be null (var alone was asked for)
template <int D, int TEAM, int ITEMS>
__device__ __forceinline__ void smooth_moments(const double (&w)[ITEMS], const double (&xp)[ITEMS][D], int cnt, int tl, double (*s_t)[2],
                                               double* __restrict__ mean_o, double* __restrict__ var_o)
{
    constexpr bool PAIR = D > 1;                                   // (D = 1: the tree's second value only ever adds +0.0)
#pragma unroll
    for (int c = 0; c < D; c += 2) {
        double x0[ITEMS], x1[ITEMS], t0[ITEMS], t1[ITEMS];
#pragma unroll
        for (int k = 0; k < ITEMS; ++k) {
            const bool in = ITEMS * tl + k < cnt;
            x0[k] = in ? xp[k][c] : 0.0;
            x1[k] = in && PAIR ? xp[k][c + (PAIR ? 1 : 0)] : 0.0;
            t0[k] = in ? w[k] * x0[k] : 0.0;
            t1[k] = in ? w[k] * x1[k] : 0.0;
        }
        double mu[2] = {lane_tree<ITEMS>(t0), lane_tree<ITEMS>(t1)};
        team_tree2<TEAM>(mu, s_t);
        if (mean_o && tl == 0) { mean_o[c] = mu[0]; if (PAIR) mean_o[c + 1] = mu[1]; }
        if (var_o) {                                               // (grid-uniform)
#pragma unroll
            for (int k = 0; k < ITEMS; ++k) {
                const bool in = ITEMS * tl + k < cnt;
                double d0 = x0[k] - mu[0], d1 = x1[k] - mu[1];
                d0 = d0 * d0; d1 = d1 * d1;
                t0[k] = in ? w[k] * d0 : 0.0;
                t1[k] = in ? w[k] * d1 : 0.0;
            }
            double s2[2] = {lane_tree<ITEMS>(t0), lane_tree<ITEMS>(t1)};
            team_tree2<TEAM>(s2, s_t);
            if (tl == 0) { var_o[c] = s2[0]; if (PAIR) var_o[c + 1] = s2[1]; }
        }
    }
}
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
// the lane's ITEMS rows of a block's snapshot (zeros beyond the block)
template <int D, int ITEMS>
__device__ __forceinline__ void smooth_load_rows(const double* __restrict__ rows_blk, int cnt, int tl, double (&xp)[ITEMS][D])
{
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
        const int i = ITEMS * tl + k;
        if (i < cnt) load_latent<D>(rows_blk + (size_t)i * D, xp[k]);
        else {
#pragma unroll
            for (int c = 0; c < D; ++c) xp[k][c] = 0.0;
        }
    }
}
// the whole walk of final block blk with the parameter row P (a kernarg array or a row of blk_params: read with constant indices only).  Args = SmoothArgs
// or PairArgs; under if constexpr each kernel keeps its own statements (tools/isa_diff.py: a kernel of this family keeps its code only if they do)
template <int M, int TEAM, int ITEMS, class Args>
__device__ __forceinline__ void block_store_walk(const Args& a, const double* P, int64_t blk, int tl, const SmoothLds& L)
{
    using Mo = Model<M>;
    constexpr bool PAIRS = std::is_same<Args, PairArgs>::value;
    constexpr int D = Mo::D, NB = PAIRS ? pairs_nb(ITEMS) : smooth_nb(ITEMS);
    const int64_t nb = a.nb;
    const int n_steps = a.hi0 - a.lo0 + 1;
    double* const mean_b = a.mean ? a.mean + blk * n_steps * D : nullptr;
    double *var_b = nullptr, *w_b = nullptr, *sec_b = nullptr, *cross_b = nullptr;
    if constexpr (PAIRS) {
        sec_b = a.second ? a.second + blk * n_steps * (D * D) : nullptr;
        cross_b = a.cross ? a.cross + blk * (n_steps - 1) * (D * D) : nullptr;
    } else {
        var_b = a.var ? a.var + blk * n_steps * D : nullptr;
        w_b = a.wout ? a.wout + blk * n_steps * nb : nullptr;
    }
    int64_t* const c_b = a.blocks ? a.blocks + blk * n_steps : nullptr;
    // the steps lo0 .. top of this block have no value, and no pair whose lower step is one of them: NaN everywhere, lineage 0
    auto undefined = [&](int top) {
        const int ns = (top < a.hi0 ? top : a.hi0) - a.lo0 + 1;
        if constexpr (PAIRS) {
            const int np = (top < a.hi0 - 1 ? top : a.hi0 - 1) - a.lo0 + 1;
            if (mean_b) for (int t = tl; t < ns * D; t += TEAM) mean_b[t] = __builtin_nan("");
            if (sec_b) for (int t = tl; t < ns * D * D; t += TEAM) sec_b[t] = __builtin_nan("");
            if (cross_b) for (int t = tl; t < np * D * D; t += TEAM) cross_b[t] = __builtin_nan("");
        } else {
            for (int t = tl; t < ns * D; t += TEAM) { if (mean_b) mean_b[t] = __builtin_nan(""); if (var_b) var_b[t] = __builtin_nan(""); }
            if (w_b) for (int64_t t = tl; t < (int64_t)ns * nb; t += TEAM) w_b[t] = __builtin_nan("");
        }
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
            if constexpr (PAIRS) {
                if (mean_b) smooth_moments<D, TEAM, ITEMS>(w, xp, cnt, tl, L.s_t, mean_b + o * D, nullptr);
                if (sec_b) pairs_products<true, D, TEAM, ITEMS>(w, xp, xp, cnt, tl, L.s_t, sec_b + o * (D * D));
            } else {
                if (mean_b || var_b) smooth_moments<D, TEAM, ITEMS>(w, xp, cnt, tl, L.s_t, mean_b ? mean_b + o * D : nullptr, var_b ? var_b + o * D : nullptr);
                if (w_b) {
#pragma unroll
                    for (int k = 0; k < ITEMS; ++k) { const int i = ITEMS * tl + k; if (i < nb) w_b[(int64_t)o * nb + i] = i < cnt ? w[k] : 0.0; }
                }
            }
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
        double lwc[ITEMS], acc[ITEMS], A[PAIRS ? ITEMS : 1][D];    // (A: the pairs' sums only)
#pragma unroll
        for (int k = 0; k < ITEMS; ++k) {
            const int i = ITEMS * tl + k;
            lwc[k] = i < ccnt ? plw[i] : -__builtin_huge_val(); acc[k] = 0.0;
            if constexpr (PAIRS) {
#pragma unroll
                for (int cc = 0; cc < D; ++cc) A[k][cc] = 0.0;
            }
        }
        const bool pair = PAIRS && cross_b && q <= a.hi0;          // (kernel-uniform: the pair (q - 1, q) is written)
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
            double lwa[NB][ITEMS], xr[PAIRS ? NB : 1][D];          // (the pairs keep a round's target rows for A; else one row at a time)
#pragma unroll
            for (int t = 0; t < NB; ++t) {
                const int j = j0 + t < cnt ? j0 + t : j0;          // (beyond the block: W = 0, any row)
                double (&xrt)[D] = xr[PAIRS ? t : 0];
                load_latent<D>(xt + (size_t)j * D, xrt);
#pragma unroll
                for (int k = 0; k < ITEMS; ++k) {
                    lwa[t][k] = -__builtin_huge_val();
                    if (ITEMS * tl + k < ccnt) lwa[t][k] = lwc[k] + Mo::logtrans(P, xp[k], xrt, ob);
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
            // ---- W_s^i (and A_i) in ascending j; invalid ancestor weights (f_j != 0, team-uniform): the whole mass of the target goes to its recorded parent
#pragma unroll
            for (int t = 0; t < NB; ++t) {
                if constexpr (PAIRS) {
                    if (Wj[t] != 0.0) {                            // (team-uniform: a dead target of a live round is skipped entirely)
                        const double Dd = (double)Dj[t];
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
                } else if (fj[t] == 0) {                           // (team-uniform; no guard on Wj: adding +0.0 to acc changes no bit)
                    const double Dd = (double)Dj[t];
#pragma unroll
                    for (int k = 0; k < ITEMS; ++k) { const double r = (double)qv[t][k] / Dd; const double term = Wj[t] * r; acc[k] = acc[k] + term; }
                } else {
                    const int j = j0 + t < cnt ? j0 + t : j0;
                    const int pl = (int)((g ? (int64_t)g[c0 + j] : c0 + j) - cp0);
#pragma unroll
                    for (int k = 0; k < ITEMS; ++k) { const double r = ITEMS * tl + k == pl ? 1.0 : 0.0; const double term = Wj[t] * r; acc[k] = acc[k] + term; }
                }
            }
        }
        if constexpr (PAIRS) {
            if (pair) pairs_products<false, D, TEAM, ITEMS>(acc, xp, A, ccnt, tl, L.s_t, cross_b + (q - 1 - a.lo0) * (D * D));
        }
#pragma unroll
        for (int k = 0; k < ITEMS; ++k) w[k] = acc[k];
        c = cp; c0 = cp0; cnt = ccnt;
    }
}
template <int M, int TEAM, int ITEMS>
__global__ __launch_bounds__(BLOCK) void k_block_smooth(SmoothArgs a, AncArgs x)
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
    if (x.blk_params) block_store_walk<M, TEAM, ITEMS>(a, x.blk_params + blk * MAX_PARAMS, blk, tl, L);     // (team-uniform)
    else block_store_walk<M, TEAM, ITEMS>(a, x.P, blk, tl, L);
}
// (the same body: written out, because as a shared __device__ function it changed k_block_smooth's code -- profiles/block_store_walk.md)
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
    if (x.blk_params) block_store_walk<M, TEAM, ITEMS>(a, x.blk_params + blk * MAX_PARAMS, blk, tl, L);     // (team-uniform)
    else block_store_walk<M, TEAM, ITEMS>(a, x.P, blk, tl, L);
}

} // namespace gpf
