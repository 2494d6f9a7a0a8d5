// K11k: a whole series per block in one launch, recording the block-wise trajectory store  (part of gpf_kernels.hpp; include that header, not this file)
#pragma once

namespace gpf {
// ----------------------------------------------------------------------------- the filter loop of many small filters with a store, block by block
// gpf_run_blocks_history (gpf.h): gpf_run_blocks' loop on a filter with the block-wise trajectory store,
//     for t in 1:T;  pf_resample_blocks(state, bs, method, ess_frac, check = false);  pf_update_blocks(state, ..., ys[:, t], bs);  end
// in ONE launch, one team per block as in k_block_run (gpf_k_block_run.hpp), whose gate, order, CDFs, search, propagate, summary and barrier
// (run_summary, run_sync) these are, statement for statement.  What is this kernel's own is what the loop's store does between the two calls of an
// iteration -- hist_on_resample's compose launch and hist_begin_step's snapshot launches (libgpf_core.hip) -- done with stores alone: iteration t works
// on store step s = s0 + t, and at the moment the slot holds its ancestor's row in registers (between the search and Model::sample)
//   the snapshot    the row's D latent columns go to hx[s][(b0 + j) D ..], in 16-byte pieces where D is even: the step's final order, after this
//                   iteration's resample and before its propagate.  A block that does not resample propagates in place, and its slot holds its OWN row
//                   here, before it overwrites it: nothing is read twice and there is no in-place hazard;
//   the weight      WEIGHTS: the log-weight pf_resample_blocks leaves the slot -- the block's average where it resampled, else its own -- to hlw[s][b0 + j];
//   the map         g = b0 + anc where the block resampled, b0 + j where not: one 4-byte store to maps[s][b0 + j].  Only at t = 0 with a composed map B
//                   already on step s0 (a gpf_resample_across_blocks came before) the word is B[g]: one dependent load through memory the launch does
//                   not write -- the new map is a fresh buffer (k_hist_compose_blocks never composes in place either);
//   the observation WEIGHTS: the first MAX_OBS lanes of the team write the block's row the step was ENTERED with to hobs[s][blk]: at t = 0 the handle's
//                   blk_obs row as it stands (obs0; the host copies it where step s0 was entered under another block size), at t > 0 the series' row
//                   t - 1, zero-padded.  blk_obs is written by the same lanes behind the loop, as in k_block_run.
// The slab and map pointers come from the store's own device tables (hist_dev_x / _lw / _obs / _maps of the handle), read with the team-uniform step
// index: a scalar load per step and table.  Nothing recorded is read inside the launch, so there is no synchronisation beyond k_block_run's.
struct RunHistArgs {
    double* const* hx;                             // [>= s0 + n_steps] the steps' snapshots, [n][D]
    double* const* hlw;                            // ... their log-weights [n] (WEIGHTS)
    double* const* hobs;                           // ... their observation rows [nblocks][MAX_OBS] (WEIGHTS)
    int32_t* const* maps;                          // ... their ancestor maps [n]
    const int32_t* map0;                           // the composed map step s0 has on entry, or null
    int32_t s0;                                    // the store's current step on entry
    int32_t obs0;                                  // WEIGHTS: the kernel writes step s0's observation rows (it was entered with this block size)
};
template <int M, int W, int METHOD, int TEAM, int ITEMS, bool WEIGHTS>
__global__ __launch_bounds__(BLOCK) void k_block_run_hist(RunArgs a, RunHistArgs hs)
{
    using Mo = Model<M>;
    constexpr int D = Mo::D;
    constexpr int TEAMS = BLOCK / TEAM, CAP = TEAM * ITEMS;
    static_assert(TEAM == WAVE || TEAM == BLOCK, "a wave or the workgroup");
    static_assert(W >= D && W % 2 == 0, "rows are moved as 16-byte column pairs");
    __shared__ uint64_t s_cdf_[BLOCK * ITEMS];
    __shared__ uint64_t s_aux_[METHOD == 0 ? 1 : BLOCK * ITEMS];
    __shared__ uint16_t s_idx_[METHOD == 2 ? BLOCK * ITEMS : 1];
    __shared__ uint64_t s_x[NWAVES][4];
    __shared__ double s_m[NWAVES];
    __shared__ int s_f[NWAVES];
    const int tm = (int)threadIdx.x / TEAM, tl = (int)threadIdx.x % TEAM;
    const int64_t blk = (int64_t)blockIdx.x * TEAMS + tm;
    if (TEAM != BLOCK && blk >= a.nblocks) return;
    uint64_t* const s_cdf = s_cdf_ + tm * CAP;
    uint64_t* const s_aux = s_aux_ + (METHOD == 0 ? 0 : tm * CAP);
    uint16_t* const s_idx = s_idx_ + (METHOD == 2 ? tm * CAP : 0);
    const int64_t b0 = blk * a.nb;
    const int cnt = (int)(a.n - b0 < a.nb ? a.n - b0 : a.nb);
    const int K = fix_K(cnt);
    const double* const P = a.blk_params ? a.blk_params + blk * MAX_PARAMS : a.P;
    const double* const obs_b = a.obs + (a.obs_blocks == 1 ? 0 : (size_t)blk * (size_t)a.n_steps * (size_t)a.n_obs);
    const double lml0 = *a.lml_est;
    double* const lw = a.lw + b0;
    int side = 0, flags_all = 0;
    double m; int f; uint64_t q[ITEMS]; uint64_t S_w; double ess;
    run_summary<TEAM, ITEMS>(lw, cnt, K, tl, s_m, s_f, s_x, m, f, q, S_w, ess);
#pragma unroll 1
    for (int t = 0; t < a.n_steps; ++t) {
        // ================ k_block_resample<METHOD>, epoch E + 2t (k_block_run's statements)
        const uint32_t ep_r = a.epoch + 2u * (uint32_t)t, ep_u = ep_r + 1u;
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
        // ================ the slots: ancestor (resample), the store's records of step s, then k_step's default proposal under epoch E + 2t + 1
        double ob[MAX_OBS];
        {
            const double* const orow = obs_b + (size_t)t * (size_t)a.n_obs;
#pragma unroll
            for (int k = 0; k < MAX_OBS; ++k) ob[k] = k < a.n_obs ? orow[k] : 0.0;
        }
        const int s = hs.s0 + t;                                   // (team-uniform: the four table reads are scalar loads)
        double* const hx = hs.hx[s] + b0 * D;
        int32_t* const hmap = hs.maps[s] + b0;
        const int32_t* const map0 = t == 0 ? hs.map0 : nullptr;
        double* hlw = nullptr;
        if (WEIGHTS) {
            hlw = hs.hlw[s] + b0;
            // the observation row the step was entered with: the handle's at t = 0, the series' row t - 1 afterwards
            if (tl < MAX_OBS && (t > 0 || hs.obs0))
                hs.hobs[s][blk * MAX_OBS + tl] = t == 0 ? a.blk_obs[blk * MAX_OBS + tl] : (tl < a.n_obs ? obs_b[(size_t)(t - 1) * (size_t)a.n_obs + tl] : 0.0);
        }
        const double* const rows_in = a.rows[side] + b0 * W;
        double* const rows_out = a.rows[go ? 1 - side : side] + b0 * W;
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
                a.anc[b0 + j] = anc;
            }
            double r[W];
            {
                const double2* src = reinterpret_cast<const double2*>(rows_in + (size_t)anc * W);
#pragma unroll
                for (int c = 0; c < (D + 1) / 2; ++c) { const double2 v = src[c]; r[2 * c] = v.x; r[2 * c + 1] = v.y; }
            }
            const double lw_in = go ? new_lw : lw[j];
            // ---- the store: step s's records of slot j, from the registers the propagate reads
            {
                const int32_t g = (int32_t)(b0 + anc);             // (anc = j where the block did not resample)
                hmap[j] = map0 ? map0[g] : g;
                if (D % 2 == 0) {
                    double2* dst = reinterpret_cast<double2*>(hx + (size_t)j * D);
#pragma unroll
                    for (int c = 0; c < D / 2; ++c) dst[c] = make_double2(r[2 * c], r[2 * c + 1]);
                } else {
#pragma unroll
                    for (int k = 0; k < D; ++k) hx[(size_t)j * D + k] = r[k];
                }
                if (WEIGHTS) hlw[j] = lw_in;
            }
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
        run_sync<TEAM>();
        // ================ k_block_stats: step t's outputs, step t + 1's gate and weights
        run_summary<TEAM, ITEMS>(lw, cnt, K, tl, s_m, s_f, s_x, m, f, q, S_w, ess);
        if (tl == 0) {
            a.ess_out[(int64_t)t * a.nblocks + blk] = f ? __builtin_nan("") : ess;
            a.lml_out[(int64_t)t * a.nblocks + blk] = (lml0 + lse_from(m, S_w, K, f)) - log_((double)cnt);
        }
    }
    if (tl == 0) a.flags_out[blk] = flags_all << 8;
    if (tl < MAX_OBS)
        a.blk_obs[blk * MAX_OBS + tl] = tl < a.n_obs ? obs_b[(size_t)(a.n_steps - 1) * (size_t)a.n_obs + tl] : 0.0;
    if (side)
        for (int e = tl; e < cnt * (W / 2); e += TEAM)
            reinterpret_cast<double2*>(a.rows[0] + b0 * W)[e] = reinterpret_cast<const double2*>(a.rows[1] + b0 * W)[e];
}

} // namespace gpf
