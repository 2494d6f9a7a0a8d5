// K11e: the most probable path per block over the trajectory store  (part of gpf_kernels.hpp; include that header, not this file)
#pragma once

namespace gpf {
// ----------------------------------------------------------------------------- particle Viterbi, block by block
// gpf_block_map_path (gpf.h; Godsill, Doucet & West 2001, "Maximum a posteriori sequence estimation using Monte Carlo particle filters", Ann. Inst.
// Statist. Math. 53; DESIGN.md 5.9 is the definition): dynamic programming in max-plus form over the grid the store holds -- the particles of the
// lineage of final block b at the steps 1 .. T.  Nothing is drawn and no weight is read.  ONE launch for all blocks and steps; one team per FINAL
// block, steps outer and descending as in block_store_walk (0-based step q below = step s = q + 1 of gpf.h):
//   lineage   block_store_walk's: c_T = b, c_s the block ALL recorded parents of block c_{s+1} sit in.  Undefined at any step: the whole block reads
//             NaN paths, index 0, logp NaN (a DP that cannot reach step 1 has no prior term) -- the team returns at that step.
//   node      n_s^i = loglik(P_b, x_s^i, obs_s[c_s]), for s >= 2 and HAS_TRANS_REST + transrest(P_b, x_s^i, obs_s[c_s]) (one add).
//   step      v_T = n_T.  The candidates i of block c_s sit ITEMS per lane in registers (rows, best, ptr); v_{s+1} is staged in LDS ([CAP] doubles);
//             the targets' rows and the observation row are team-uniform addresses.  Lane-private, ascending j:
//                 val = logtrans(P_b, x_s^i, x_{s+1}^j, obs_{s+1}[c_{s+1}]) + v_{s+1}^j;    if (val > best) { best = val; ptr = j; }
//             from best = -Inf, ptr = 0: a NaN never wins, the smallest j wins a tie.  v_s^i = n_s^i + best.  NO reduction per target: the team's only
//             reductions are the lineage check per step and the arg-max at step 1; two team syncs per step order the LDS copy of v.
//   pointers  ptr_s[i] as 16-bit words in device scratch of the call, [T - 1][nblocks][bsp] by the FINAL block (two final blocks may share a lineage
//             block), bsp = the block size rounded up to a multiple of 8: a lane stores its ITEMS consecutive entries with ONE 4- or 16-byte store.  The lineage
//             blocks c_s go to [nblocks][T] words beside them (lane 0).
//   step 1    tot_i = logprior(P_b, x_1^i, obs_1[c_1]) + v_1^i; (maximum of the non-NaN totals, smallest i attaining it) over the team.
//   trace     the SAME launch: after a team sync (the team's own pointer stores are visible to its lane 0: one CU, workgroup scope) lane 0 follows
//             p_1 = i*, p_{s+1} = ptr_s[p_s] -- T - 1 dependent 2-byte loads, L2 hits of lines the team has just written -- and writes the rows and
//             indices of the steps in [lo0, hi0].  A second launch would add a launch for the same chain and need i* in memory.
// P_b: the FINAL block's row of blk_params where per-block parameters are set, else the filter's (as k_block_smooth).
// Outputs (any may be null), n_steps = hi0 - lo0 + 1: path = [nblocks][n_steps][D], idx = [nblocks][n_steps] 1-based global, logp = [nblocks].
struct MapArgs : StoreWalkArgs {
    double* path; int64_t* idx; double* logp;
    uint16_t* ptr;                                 // [T - 1][nblocks][bsp] scratch, 16-byte aligned rows
    int32_t* lin;                                  // [nblocks][T] scratch: the lineage blocks
    int64_t bsp;                                   // nb rounded up to a multiple of 8
};
struct MapLds {
    double* V;                                     // [CAP] v of the targets' step
    int (*s_c)[2];                                 // the lineage check's words
    double* s_m; int (*s_i)[2];                    // the arg-max's words (TEAM = BLOCK only)
};
template <int M, int TEAM, int ITEMS>
__device__ __forceinline__ void block_map_walk(const MapArgs& a, const double* P, int64_t blk, int tl, const MapLds& L)
{
    using Mo = Model<M>;
    constexpr int D = Mo::D;
    static_assert(ITEMS == 2 || ITEMS == 8, "a lane's pointers are one 4- or 16-byte store");
    const int64_t nb = a.nb;
    const int n_steps = a.hi0 - a.lo0 + 1;
    double* const path_b = a.path ? a.path + blk * n_steps * D : nullptr;
    int64_t* const idx_b = a.idx ? a.idx + blk * n_steps : nullptr;
    // no path: NaN rows, index 0
    auto no_path = [&](double lp) {
        if (path_b) for (int t = tl; t < n_steps * D; t += TEAM) path_b[t] = __builtin_nan("");
        if (idx_b) for (int t = tl; t < n_steps; t += TEAM) idx_b[t] = 0;
        if (a.logp && tl == 0) a.logp[blk] = lp;
    };
    auto node = [&](const double (&x)[D], const double (&ob)[MAX_OBS], int q) {
        const double ll = Mo::loglik(P, x, ob);
        if constexpr (Mo::HAS_TRANS_REST) { if (q >= 1) return ll + Mo::transrest(P, x, ob); }
        return ll;
    };
    int32_t* const lin_b = a.lin + blk * a.T;
    int64_t c = blk, c0 = c * nb;
    int cnt = (int)(a.n - c0 < nb ? a.n - c0 : nb);
    // ---- step T: v = n
    double xp[ITEMS][D], v[ITEMS], ob[MAX_OBS];
    smooth_load_rows<D, ITEMS>(a.hx[a.T - 1] + c0 * D, cnt, tl, xp);
    {
        const double* __restrict__ orow = a.hobs[a.T - 1] + (size_t)c * MAX_OBS;
#pragma unroll
        for (int k = 0; k < MAX_OBS; ++k) ob[k] = orow[k];
    }
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) v[k] = node(xp[k], ob, a.T - 1);
    if (tl == 0) lin_b[a.T - 1] = (int32_t)c;
    for (int q = a.T - 1; q >= 1; --q) {
        // ---- the lineage: the block all recorded parents of block c sit in (block_store_walk's statements)
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
        if (bmin != bmax) { no_path(__builtin_nan("")); return; }  // (team-uniform)
        // ---- v of the targets to LDS (the entries beyond the block are never read); the candidates of step q - 1 to registers
        team_sync<TEAM>();                                         // (the previous step's loop has read L.V)
#pragma unroll
        for (int k = 0; k < ITEMS; ++k) L.V[ITEMS * tl + k] = v[k];
        team_sync<TEAM>();
        const int64_t cp = bmin, cp0 = cp * nb;
        const int ccnt = (int)(a.n - cp0 < nb ? a.n - cp0 : nb);
        smooth_load_rows<D, ITEMS>(a.hx[q - 1] + cp0 * D, ccnt, tl, xp);
        const double* __restrict__ xt = a.hx[q] + c0 * D;          // the targets' rows: one broadcast address each; ob is still obs_{q}[c]
        double best[ITEMS]; int ptr[ITEMS];
#pragma unroll
        for (int k = 0; k < ITEMS; ++k) { best[k] = -__builtin_huge_val(); ptr[k] = 0; }
#pragma unroll 2
        for (int j = 0; j < cnt; ++j) {
            double xr[D];
            load_latent<D>(xt + (size_t)j * D, xr);
            const double vj = L.V[j];
#pragma unroll
            for (int k = 0; k < ITEMS; ++k) {
                const double val = Mo::logtrans(P, xp[k], xr, ob) + vj;
                if (val > best[k]) { best[k] = val; ptr[k] = j; }
            }
        }
        // ---- the candidates' own step: its observation row, v = n + best; the pointers, ITEMS consecutive entries per lane in one store
        {
            const double* __restrict__ orow = a.hobs[q - 1] + (size_t)cp * MAX_OBS;
#pragma unroll
            for (int k = 0; k < MAX_OBS; ++k) ob[k] = orow[k];
        }
#pragma unroll
        for (int k = 0; k < ITEMS; ++k) v[k] = node(xp[k], ob, q - 1) + best[k];
        if (ITEMS * tl < ccnt) {                                   // (ITEMS * tl + ITEMS <= bsp: the row is padded to a multiple of 8)
            uint16_t* const dst = a.ptr + ((size_t)(q - 1) * (size_t)a.nblocks + (size_t)blk) * (size_t)a.bsp + (size_t)(ITEMS * tl);
            if constexpr (ITEMS == 2) *reinterpret_cast<uint32_t*>(dst) = (uint32_t)ptr[0] | ((uint32_t)ptr[1] << 16);
            else {
                uint4 w;
                w.x = (uint32_t)ptr[0] | ((uint32_t)ptr[1] << 16); w.y = (uint32_t)ptr[2] | ((uint32_t)ptr[3] << 16);
                w.z = (uint32_t)ptr[4] | ((uint32_t)ptr[5] << 16); w.w = (uint32_t)ptr[6] | ((uint32_t)ptr[7] << 16);
                *reinterpret_cast<uint4*>(dst) = w;
            }
        }
        if (tl == 0) lin_b[q - 1] = (int32_t)cp;
        c = cp; c0 = cp0; cnt = ccnt;
    }
    // ---- step 1: the prior term; the maximum of the non-NaN totals and the smallest index that attains it
    double m = -__builtin_huge_val(); int some = 0;
    double tot[ITEMS];
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
        tot[k] = Mo::logprior(P, xp[k], ob) + v[k];
        if (ITEMS * tl + k < cnt && tot[k] == tot[k]) { some = 1; m = tot[k] > m ? tot[k] : m; }
    }
    m = wave_max_f64(m);
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) some |= __shfl_xor(some, s, WAVE);
    if (TEAM == BLOCK) {
        if (lane_id() == 0) { L.s_m[wave_id()] = m; L.s_i[wave_id()][0] = some; }
        __syncthreads();
#pragma unroll
        for (int w = 0; w < NWAVES; ++w) { m = L.s_m[w] > m ? L.s_m[w] : m; some |= L.s_i[w][0]; }
    }
    int ist = 0x7fffffff;
#pragma unroll
    for (int k = ITEMS - 1; k >= 0; --k) if (ITEMS * tl + k < cnt && tot[k] == m) ist = ITEMS * tl + k;
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) { const int o = __shfl_xor(ist, s, WAVE); ist = o < ist ? o : ist; }
    if (TEAM == BLOCK) {
        if (lane_id() == 0) L.s_i[wave_id()][1] = ist;
        __syncthreads();
#pragma unroll
        for (int w = 0; w < NWAVES; ++w) ist = L.s_i[w][1] < ist ? L.s_i[w][1] : ist;
    }
    if (!some) { no_path(__builtin_nan("")); return; }             // (team-uniform) every total NaN
    if (m == -__builtin_huge_val()) { no_path(m); return; }        // no path of positive density on the grid
    // ---- the trace: lane 0 follows the team's own pointers
    __threadfence_block();
    team_sync<TEAM>();
    if (tl != 0) return;
    if (a.logp) a.logp[blk] = m;
    if (!path_b && !idx_b) return;
    int p = ist;
    for (int q = 0; q < a.T && q <= a.hi0; ++q) {
        if (q >= a.lo0) {
            const int64_t gi = (int64_t)lin_b[q] * nb + p;
            const int o = q - a.lo0;
            if (path_b) {
                double xr[D];
                load_latent<D>(a.hx[q] + gi * D, xr);
#pragma unroll
                for (int cc = 0; cc < D; ++cc) path_b[o * D + cc] = xr[cc];
            }
            if (idx_b) idx_b[o] = gi + 1;
        }
        if (q + 1 < a.T) p = (int)a.ptr[((size_t)q * (size_t)a.nblocks + (size_t)blk) * (size_t)a.bsp + (size_t)p];
    }
}
template <int M, int TEAM, int ITEMS>
__global__ __launch_bounds__(BLOCK) void k_block_map(MapArgs a, AncArgs x)
{
    constexpr int TEAMS = BLOCK / TEAM, CAP = TEAM * ITEMS;
    static_assert(TEAM == WAVE || TEAM == BLOCK, "a wave or the workgroup");
    static_assert(Model<M>::D == 1 || Model<M>::D == 2 || Model<M>::D == 4, "the latent columns are moved as words or 16-byte pairs");
    __shared__ double s_V[BLOCK * ITEMS];
    __shared__ int s_c[NWAVES][2];
    __shared__ double s_m[NWAVES];
    __shared__ int s_i[NWAVES][2];
    const int tm = (int)threadIdx.x / TEAM, tl = (int)threadIdx.x % TEAM;
    const int64_t blk = (int64_t)blockIdx.x * TEAMS + tm;
    if (TEAM != BLOCK && blk >= a.nblocks) return;                 // (an idle wave: the wave-team path has no workgroup barrier)
    const MapLds L{s_V + tm * CAP, s_c, s_m, s_i};
    if (x.blk_params) block_map_walk<M, TEAM, ITEMS>(a, x.blk_params + blk * MAX_PARAMS, blk, tl, L);       // (team-uniform)
    else block_map_walk<M, TEAM, ITEMS>(a, x.P, blk, tl, L);
}

} // namespace gpf
