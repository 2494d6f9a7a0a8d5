// K11: block-wise resampling -- many small filters in one launch  (part of gpf_kernels.hpp; include that header, not this file)
#pragma once

namespace gpf {
// ----------------------------------------------------------------------------- K11: one workgroup = one block of particles
// The reference runs many small filters in one state as sub-states: `for b in blocks; pf_resample!(state[b], method); end`
// (src/view.jl:16-48, the block-wise resampling of test/resample.jl:130-162; README.md:60-79 and every reference test run
// N = 100).  Through the single-filter path that is one view and three to five launches per block, ~18 us each time however small the
// block.  Here ONE launch does the loop: workgroup b owns the particles [b nb, min((b + 1) nb, n)), nb <= 2048, and runs the
// whole resample of that sub-state out of LDS -- maximum and validity flags (safe_softmax, utils.jl:117-140), K-bit fixed-point
// weights (K from the BLOCK's particle count, like a view), their exact CDF, optionally the stable descending order
// (sort_particles, resample.jl:156-157: bitonic network over (key, index) pairs), the ancestors of the block's slots by
// binary search (multinomial :59, residual :96-115, stratified :159-168), the row gather (:60) and the sub-state weight update
// (every particle gets logsumexp(block weights) - log(block size), :205-211).  RNG counters are the slots' global ids and the
// call's epoch, so block b's result is bit-identical to pf_resample!(state[b]) through a view, and to the oracle's sub-state
// resample.  ess_frac >= 0: a block resamples only if its effective sample size is below ess_frac x (block size) -- the
// `if effective_sample_size(state) < N / 2` of the README loop, decided per block on the device (no host round trip).
// Teams: a block of up to 512 particles is the work of ONE WAVE (TEAM = 64, 2 or 8 consecutive particles per lane, four blocks per
// workgroup, no workgroup barrier anywhere: LDS operations of one wave execute in order), a larger one of the whole workgroup
// (TEAM = 256, 8 per lane).  10^4 blocks of 100 particles: 105 us with a workgroup per block, profiles/r03_small_filters.txt for the rest.
constexpr int BLK_MAX = 2048;                      // particles per block
struct BlockArgs {
    const double* rows_in; double* rows_out;       // [n][W]
    double* lw;                                    // [n] log-weights, rewritten for the blocks that resample
    int32_t* anc;                                  // [n] parents, LOCAL to the block (0-based), rewritten for the blocks that resample
    int64_t n, nb;                                 // particles, particles per block
    int64_t nblocks;
    int64_t gid0;                                  // global id of particle 0 (RNG counters)
    uint64_t seed; uint32_t epoch;
    int sorted;                                    // stratified: sort_particles
    double alpha;                                  // PRIO kernels: priority_fn = w -> alpha w (resample.jl:51-52)
    double ess_frac;                               // < 0: every block resamples
    int check_true;                                // check = true: blocks with invalid (all -Inf) weights are left alone as well
    int32_t* resampled;                            // [n_blocks] bit 0: the block resampled; bits 8..: its validity flags (no shared counter:
                                                   // 10^4 same-address atomics would cost ~100 us; k_block_summary folds the words on request)
};
// OR of the blocks' flags and the number of blocks that resampled -> out2 = {flags, count}
static __global__ __launch_bounds__(BLOCK) void k_block_summary(const int32_t* __restrict__ words, int64_t nblocks, int32_t* __restrict__ out2)
{
    int f = 0; unsigned c = 0;
    for (int64_t i = threadIdx.x; i < nblocks; i += BLOCK) { const int w = words[i]; f |= w >> 8; c += (unsigned)(w & 1); }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) { f |= __shfl_xor(f, s, WAVE); c += (unsigned)__shfl_xor((int)c, s, WAVE); }
    __shared__ int s_f[NWAVES]; __shared__ unsigned s_c[NWAVES];
    if (lane_id() == 0) { s_f[wave_id()] = f; s_c[wave_id()] = c; }
    __syncthreads();
    if (threadIdx.x == 0) { for (int w = 1; w < NWAVES; ++w) { f |= s_f[w]; c += s_c[w]; } out2[0] = f; out2[1] = (int32_t)c; }
}

template <int TEAM>
__device__ __forceinline__ void team_sync()
{
    if (TEAM == BLOCK) __syncthreads();
    else { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); }
}
// sums of four words over the team; s_x: [NWAVES][4] words of LDS (TEAM = BLOCK only)
template <int TEAM>
__device__ __forceinline__ void team_sum4(uint64_t (&v)[4], uint64_t (*s_x)[4])
{
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] = wave_sum_u64(v[c]);
    if (TEAM == BLOCK) {
        __syncthreads();
        if (lane_id() == 0) { for (int c = 0; c < 4; ++c) s_x[wave_id()][c] = v[c]; }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < 4; ++c) { uint64_t t = 0; for (int w = 0; w < NWAVES; ++w) t += s_x[w][c]; v[c] = t; }
    }
}
// team-wide inclusive scan of ITEMS consecutive values per lane; returns the total.  s_x: LDS scratch as above
template <int TEAM, int ITEMS>
__device__ __forceinline__ uint64_t team_scan_incl(uint64_t (&v)[ITEMS], uint64_t (*s_x)[4])
{
#pragma unroll
    for (int k = 1; k < ITEMS; ++k) v[k] += v[k - 1];
    const uint64_t inc = wave_scan_u64(v[ITEMS - 1]);              // inclusive over the lanes' totals
    uint64_t pre = inc - v[ITEMS - 1], tot = shfl_u64(inc, WAVE - 1);
    if (TEAM == BLOCK) {
        __syncthreads();                                           // s_x may still be read from a previous call
        if (lane_id() == WAVE - 1) s_x[wave_id()][0] = inc;
        __syncthreads();
        tot = 0;
#pragma unroll
        for (int w = 0; w < NWAVES; ++w) { const uint64_t t = s_x[w][0]; if (w < wave_id()) pre += t; tot += t; }
    }
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) v[k] += pre;
    return tot;
}
// first index a in [0, cnt) with cdf[a] > T, clamped to cnt - 1 (the while loop of resample.jl:163-166 / inverse-CDF categorical)
__device__ __forceinline__ int lds_upper_bound(const uint64_t* cdf, int cnt, uint64_t T)
{
    int lo = 0, len = cnt;
    while (len > 0) { const int half = len >> 1; if (cdf[lo + half] <= T) { lo += half + 1; len -= half + 1; } else len = half; }
    return lo < cnt ? lo : cnt - 1;
}

// maximum and validity flags of the team's values (safe_softmax, utils.jl:119-126); s_m / s_f: NWAVES words each (TEAM = BLOCK only)
template <int TEAM, int ITEMS>
__device__ __forceinline__ void team_max_flags(const double (&v)[ITEMS], int tl, int cnt, double* s_m, int* s_f, double& m_out, int& f_out)
{
    double m = -__builtin_huge_val(); int f = 0;
#pragma unroll
    for (int k = 0; k < ITEMS; ++k)
        if (ITEMS * tl + k < cnt) { const double x = v[k]; if (x != x) f |= FLAG_NAN; else { m = x > m ? x : m; if (x == __builtin_huge_val()) f |= FLAG_POSINF; } }
    m = wave_max_f64(m);
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) f |= __shfl_xor(f, s, WAVE);
    if (TEAM == BLOCK) {
        __syncthreads();                                           // (s_m / s_f may still be read from a previous call)
        if (lane_id() == 0) { s_m[wave_id()] = m; s_f[wave_id()] = f; }
        __syncthreads();
#pragma unroll
        for (int w = 0; w < NWAVES; ++w) { m = s_m[w] > m ? s_m[w] : m; f |= s_f[w]; }
    }
    if (!(f & FLAG_NAN) && m == -__builtin_huge_val()) f |= FLAG_ALL_NEGINF;
    m_out = m; f_out = f;
}

// PRIO: priority_fn = w -> alpha w (resample.jl:51-52): ancestors from the priorities' CDF, the ESS gate on the raw weights, new weights
// log_ws + (logsumexp(block weights) - logsumexp(log_ws)) with log_ws = lw[a] - lp[a] (the sub-state form, resample.jl:213-216)
// METHOD_COND (conditional SMC, gpf_resample_blocks_conditional; Andrieu, Doucet & Holenstein 2010, the conditional multinomial step): METHOD 0 in
// which slot 0 of every block that resamples keeps local ancestor 0 -- its own row -- while the slots j >= 1 draw exactly as in METHOD 0 (same
// counters, same CDF) and every particle gets the same new weight.  A value of METHOD rather than one more template parameter: the names of the
// instantiations that existed before stay as they are.
constexpr int METHOD_COND = 3;
template <int METHOD_, int W, int TEAM, int ITEMS, bool PRIO = false>    // METHOD 0 multinomial, 1 residual, 2 stratified
__global__ __launch_bounds__(BLOCK) void k_block_resample(BlockArgs a)
{
    constexpr bool COND = METHOD_ == METHOD_COND;
    constexpr int METHOD = COND ? 0 : METHOD_;
    static_assert(!COND || !PRIO, "the conditional step is multinomial on the raw weights");
    constexpr int TEAMS = BLOCK / TEAM, CAP = TEAM * ITEMS;        // blocks per workgroup, particles a team holds
    static_assert(TEAM == WAVE || TEAM == BLOCK, "a wave or the workgroup");
    __shared__ uint64_t s_cdf_[BLOCK * ITEMS];                     // the CDF that is sampled (weights; residual: residual weights)
    __shared__ uint64_t s_aux_[METHOD == 0 ? 1 : BLOCK * ITEMS];   // residual: copy-count CDF; stratified: sort keys
    __shared__ uint16_t s_idx_[METHOD == 2 ? BLOCK * ITEMS : 1];   // stratified, sorted: the order
    __shared__ uint64_t s_x[NWAVES][4];
    __shared__ double s_m[NWAVES];
    __shared__ int s_f[NWAVES];
    __shared__ double s_lw_[PRIO ? BLOCK * ITEMS : 1];             // PRIO: the block's incoming log-weights, then log_ws of its slots
    __shared__ double s_lws_[PRIO ? BLOCK * ITEMS : 1];
    const int tm = (int)threadIdx.x / TEAM, tl = (int)threadIdx.x % TEAM;
    const int64_t blk = (int64_t)blockIdx.x * TEAMS + tm;
    if (TEAM != BLOCK && blk >= a.nblocks) return;                 // (an idle wave: the wave-team path has no workgroup barrier)
    double* const s_lw = s_lw_ + (PRIO ? tm * CAP : 0);
    double* const s_lws = s_lws_ + (PRIO ? tm * CAP : 0);
    uint64_t* const s_cdf = s_cdf_ + tm * CAP;
    uint64_t* const s_aux = s_aux_ + (METHOD == 0 ? 0 : tm * CAP);
    uint16_t* const s_idx = s_idx_ + (METHOD == 2 ? tm * CAP : 0);
    const int64_t b0 = blk * a.nb;
    const int cnt = (int)(a.n - b0 < a.nb ? a.n - b0 : a.nb);      // particles of this block
    const int K = fix_K(cnt);
    // ---- the raw weights: maximum + flags (utils.jl:119-126), fixed-point weights, their sum (and sum of squares for the ESS gate)
    double lwv[ITEMS];
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) { const int i = ITEMS * tl + k; lwv[k] = i < cnt ? a.lw[b0 + i] : -__builtin_huge_val(); }
    double m_r; int f_r;
    team_max_flags<TEAM, ITEMS>(lwv, tl, cnt, s_m, s_f, m_r, f_r);
    uint64_t q[ITEMS];
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) q[k] = ITEMS * tl + k < cnt ? ((f_r & FLAG_ALL_NEGINF) ? 1ull : exp_fix(lwv[k] - m_r, K)) : 0ull;
    bool gate = true;                                              // the block passes the ESS test (or there is none)
    uint64_t S_r = 0;
    if (PRIO || a.ess_frac >= 0.0) {                               // (team-uniform)
        unsigned __int128 Q = 0; uint64_t sl = 0;
#pragma unroll
        for (int k = 0; k < ITEMS; ++k) { Q += (unsigned __int128)q[k] * q[k]; sl += q[k]; }
        // 128-bit team sum by limbs: the low word in two 32-bit halves (their carries just add up)
        uint64_t v4[4] = {(uint64_t)Q & 0xffffffffull, (uint64_t)Q >> 32, (uint64_t)(Q >> 64), sl};
        team_sum4<TEAM>(v4, s_x);
        S_r = v4[3];
        if (a.ess_frac >= 0.0) {
            const unsigned __int128 Qt = ((unsigned __int128)v4[2] << 64) + ((unsigned __int128)v4[1] << 32) + v4[0];
            const double ess = ess_from(S_r, (uint64_t)(Qt >> 64), (uint64_t)Qt);
            // `effective_sample_size(state) < N / 2`, README.md:72; invalid weights: the reference's ESS is NaN and the comparison false
            gate = f_r == 0 && ess < a.ess_frac * (double)cnt;
        }
    }
    // ---- what the resampler samples from: the raw weights, or the priorities alpha * lw (their own maximum, flags, fixed-point weights)
    double m = m_r; int f = f_r;
    if (PRIO) {
#pragma unroll
        for (int k = 0; k < ITEMS; ++k) { const int i = ITEMS * tl + k; if (i < cnt) s_lw[i] = lwv[k]; lwv[k] = i < cnt ? a.alpha * lwv[k] : -__builtin_huge_val(); }
        team_max_flags<TEAM, ITEMS>(lwv, tl, cnt, s_m, s_f, m, f);
#pragma unroll
        for (int k = 0; k < ITEMS; ++k) q[k] = ITEMS * tl + k < cnt ? ((f & FLAG_ALL_NEGINF) ? 1ull : exp_fix(lwv[k] - m, K)) : 0ull;
    }
    // NaN / +Inf: Categorical rejects them in the reference; with check = true any invalid block: left as it stands
    const bool skip = (f & (FLAG_NAN | FLAG_POSINF)) != 0 || (a.check_true && f != 0);
    const bool uniform = (f & FLAG_ALL_NEGINF) != 0;
    const bool go = gate && !skip;
    // (a block that does not pass its ESS test never gets as far as safe_softmax: nothing to report for it)
    if (tl == 0) a.resampled[blk] = (go ? 1 : 0) | ((gate ? f : 0) << 8);
    if (!go) {
        // this block keeps its particles: rows move to the other buffer unchanged, weights and parents stay
        for (int t = tl; t < cnt * (W / 2); t += TEAM)
            reinterpret_cast<double2*>(a.rows_out + b0 * W)[t] = reinterpret_cast<const double2*>(a.rows_in + b0 * W)[t];
        return;
    }
    // ---- sort_particles (stratified, resample.jl:156-157): order = sortperm(log_priorities, rev = true), stable.  Bitonic network over
    //      (key, index) pairs -- the index makes every pair distinct, so the network's order IS the stable order
    if (METHOD == 2 && a.sorted) {
        int p2 = 2;                                                // the network's size: the next power of two >= cnt
        while (p2 < cnt) p2 <<= 1;
        for (int i = tl; i < p2; i += TEAM) { s_aux[i] = i < cnt ? sort_key_desc(PRIO ? a.alpha * a.lw[b0 + i] : a.lw[b0 + i]) : ~0ull; s_idx[i] = (uint16_t)i; }
        team_sync<TEAM>();
        for (int size = 2; size <= p2; size <<= 1) {
            for (int stride = size >> 1; stride >= 1; stride >>= 1) {
                for (int t = tl; t < p2 / 2; t += TEAM) {
                    const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
                    const bool up = (lo & size) == 0;
                    const uint64_t ka = s_aux[lo], kb = s_aux[hi];
                    const uint16_t ia = s_idx[lo], ib = s_idx[hi];
                    const bool gt = ka > kb || (ka == kb && ia > ib);
                    if (gt == up) { s_aux[lo] = kb; s_aux[hi] = ka; s_idx[lo] = ib; s_idx[hi] = ia; }
                }
                team_sync<TEAM>();
            }
        }
        // the weights in sorted order (the key map is a bijection: no second read of lw)
#pragma unroll
        for (int k = 0; k < ITEMS; ++k) {
            const int i = ITEMS * tl + k;
            q[k] = i < cnt ? (uniform ? 1ull : exp_fix(sort_key_value(s_aux[i]) - m, K)) : 0ull;
        }
        team_sync<TEAM>();
    }
    // ---- the CDF(s)
    uint64_t S, Ctot = 0, Rs = 0;
    if (METHOD == 1) {
        // residual (resample.jl:96-115): copies c_i = floor(N w_i) = (N q_i) div S, residual weight ((N q_i) mod S) >> sh
        uint64_t sq[ITEMS];
#pragma unroll
        for (int k = 0; k < ITEMS; ++k) sq[k] = q[k];
        S = team_scan_incl<TEAM, ITEMS>(sq, s_x);
        const int sh = residual_shift(S, cnt);
        uint64_t c[ITEMS], r[ITEMS];
#pragma unroll
        for (int k = 0; k < ITEMS; ++k) {
            // (N q) div S and mod S with a quotient <= N <= 2048: the double estimate is off by at most one, two exact corrections
            // instead of a 64-bit division
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
    // ---- ancestors, gather, sub-state weights (resample.jl:205-211: every particle carries the block's average weight)
    const double new_lw = PRIO ? 0.0 : lse_from(m, S, K, f) - log_((double)cnt);
    const uint64_t sB = METHOD == 2 ? S / (uint64_t)cnt : 0, srem = METHOD == 2 ? S % (uint64_t)cnt : 0;
    for (int j = tl; j < cnt; j += TEAM) {                         // consecutive lanes, consecutive slots: coalesced stores
        const uint32_t slot = (uint32_t)(a.gid0 + b0 + j);
        int anc;
        if (METHOD == 0) anc = lds_upper_bound(s_cdf, cnt, mulhi64(resample_u64(a.seed, slot, a.epoch), S));          // :59
        else if (METHOD == 1) {
            if ((uint64_t)j < Ctot) anc = lds_upper_bound(s_aux, cnt, (uint64_t)j);                                 // :101 (no draw)
            else anc = lds_upper_bound(s_cdf, cnt, mulhi64(resample_u64(a.seed, slot, a.epoch), Rs));               // :113
        } else {
            const uint64_t jl = (uint64_t)j;                                                               // strata are local to the block
            // (j rem < 2048^2: 32-bit divisions)
            const uint64_t L0 = jl * sB + (uint32_t)(jl * srem) / (uint32_t)cnt, L1 = (jl + 1) * sB + (uint32_t)((jl + 1) * srem) / (uint32_t)cnt;
            anc = lds_upper_bound(s_cdf, cnt, L0 + mulhi64(resample_u64(a.seed, slot, a.epoch), L1 - L0));        // :162-166
            if (a.sorted) anc = (int)s_idx[anc];                                                           // :168
        }
        if (COND && j == 0) anc = 0;                                                                       // the retained path survives
        const double2* src = reinterpret_cast<const double2*>(a.rows_in + (b0 + anc) * W);
        double2* dst = reinterpret_cast<double2*>(a.rows_out + (b0 + j) * W);
#pragma unroll
        for (int c = 0; c < W / 2; ++c) dst[c] = src[c];
        a.anc[b0 + j] = anc;
        if (PRIO) { const double w0 = s_lw[anc]; s_lws[j] = w0 - a.alpha * w0; }               // log_ws = lw[a] - lp[a]  (:213)
        else a.lw[b0 + j] = new_lw;
    }
    if (PRIO) {
        // lw = log_ws + (logsumexp(block's incoming weights) - logsumexp(log_ws))   (resample.jl:213-216)
        team_sync<TEAM>();
        double wv2[ITEMS];
#pragma unroll
        for (int k = 0; k < ITEMS; ++k) { const int i = ITEMS * tl + k; wv2[k] = i < cnt ? s_lws[i] : -__builtin_huge_val(); }
        double m2; int f2;
        team_max_flags<TEAM, ITEMS>(wv2, tl, cnt, s_m, s_f, m2, f2);
        uint64_t v4[4] = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < ITEMS; ++k) v4[3] += ITEMS * tl + k < cnt ? ((f2 & FLAG_ALL_NEGINF) ? 1ull : exp_fix(wv2[k] - m2, K)) : 0ull;
        team_sum4<TEAM>(v4, s_x);
        const double off = lse_from(m_r, S_r, K, f_r) - lse_from(m2, v4[3], K, f2);
#pragma unroll
        for (int k = 0; k < ITEMS; ++k) { const int i = ITEMS * tl + k; if (i < cnt) a.lw[b0 + i] = wv2[k] + off; }
    }
}

// per-block effective sample size and log-ML estimate of a sub-state (utils.jl:163-178): ess[b], lml[b] = (lml_est + logsumexp(block)) - log(block size);
// teams as in k_block_resample
template <int TEAM, int ITEMS>
__global__ __launch_bounds__(BLOCK) void k_block_stats(const double* __restrict__ lw, int64_t n, int64_t nb, int64_t nblocks, const double* lml_est,
                                                       double* __restrict__ ess_out, double* __restrict__ lml_out)
{
    constexpr int TEAMS = BLOCK / TEAM;
    __shared__ double s_m[NWAVES];
    __shared__ int s_f[NWAVES];
    __shared__ uint64_t s_x[NWAVES][4];
    const int tm = (int)threadIdx.x / TEAM, tl = (int)threadIdx.x % TEAM, lane = lane_id(), wv = wave_id();
    const int64_t blk = (int64_t)blockIdx.x * TEAMS + tm;
    if (TEAM != BLOCK && blk >= nblocks) return;
    const int64_t b0 = blk * nb;
    const int cnt = (int)(n - b0 < nb ? n - b0 : nb);
    const int K = fix_K(cnt);
    double lwv[ITEMS];
    double m = -__builtin_huge_val(); int f = 0;
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
        const int i = ITEMS * tl + k;
        lwv[k] = i < cnt ? lw[b0 + i] : -__builtin_huge_val();
        if (i < cnt) { const double v = lwv[k]; if (v != v) f |= FLAG_NAN; else { m = v > m ? v : m; if (v == __builtin_huge_val()) f |= FLAG_POSINF; } }
    }
    m = wave_max_f64(m);
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) f |= __shfl_xor(f, s, WAVE);
    if (TEAM == BLOCK) {
        if (lane == 0) { s_m[wv] = m; s_f[wv] = f; }
        __syncthreads();
#pragma unroll
        for (int w = 0; w < NWAVES; ++w) { m = s_m[w] > m ? s_m[w] : m; f |= s_f[w]; }
    }
    if (!(f & FLAG_NAN) && m == -__builtin_huge_val()) f |= FLAG_ALL_NEGINF;
    const bool uniform = (f & FLAG_ALL_NEGINF) != 0;
    unsigned __int128 Q = 0; uint64_t sl = 0;
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
        const uint64_t q = ITEMS * tl + k < cnt ? (uniform ? 1ull : exp_fix(lwv[k] - m, K)) : 0ull;
        Q += (unsigned __int128)q * q; sl += q;
    }
    uint64_t v4[4] = {(uint64_t)Q & 0xffffffffull, (uint64_t)Q >> 32, (uint64_t)(Q >> 64), sl};
    team_sum4<TEAM>(v4, s_x);
    if (tl == 0) {
        const unsigned __int128 Qt = ((unsigned __int128)v4[2] << 64) + ((unsigned __int128)v4[1] << 32) + v4[0];
        ess_out[blk] = f ? __builtin_nan("") : ess_from(v4[3], (uint64_t)(Qt >> 64), (uint64_t)Qt);     // (lognorm of invalid weights is NaN)
        lml_out[blk] = (*lml_est + lse_from(m, v4[3], K, f)) - log_((double)cnt);                       // utils.jl:174-178, left to right
    }
}

// ----------------------------------------------------------------------------- per-block estimates: mean / var / proportionmap of every sub-state
// for b in blocks; mean(state[b], addr); var(state[b], addr); proportionmap(state[b], addr); end (statistics.jl:13-14, 48-50, 91-101 on
// ParticleFilterSubStates, view.jl:35-48) in ONE launch for all blocks and all columns, bit-identical to gpf_mean / gpf_var / gpf_proportion on a view
// of the block.  The order of the sum is the spec's (k_wsum_tree): a block of <= 2048 particles is ONE chunk of the binary tree over
// the block-local index.  A lane holds ITEMS consecutive terms and sums them as their own subtree, the xor butterfly m = 1, 2, ..., 32 joins the 64
// lanes, the workgroup team joins its four waves as (s0 + s1) + (s2 + s3); the levels a narrower team does not have only ever add +0.0.
// Teams as in k_block_stats.  The normalised weights stay in registers; the rows are read as 16-byte column pairs (a lane's rows are one
// contiguous run -- at W = 8 the four passes over it hit in L2, a block is at most 128 KB).
template <int ITEMS>
__device__ __forceinline__ double lane_tree(const double (&t)[ITEMS])
{
    static_assert(ITEMS == 2 || ITEMS == 8, "a lane's subtree");
    if constexpr (ITEMS == 2) return t[0] + t[1];
    else return tree8(t);
}
// the tree over the team of two values at once (every thread gets the results); s_t: [NWAVES][2] words of LDS (TEAM = BLOCK only)
template <int TEAM>
__device__ __forceinline__ void team_tree2(double (&v)[2], double (*s_t)[2])
{
#pragma unroll
    for (int m = 1; m < WAVE; m <<= 1) {                             // neighbours first
        v[0] += u2d(shfl_xor_u64(d2u(v[0]), m));
        v[1] += u2d(shfl_xor_u64(d2u(v[1]), m));
    }
    if (TEAM == BLOCK) {
        static_assert(NWAVES == 4, "two more levels");
        __syncthreads();                                           // (s_t may still be read from a previous call)
        if (lane_id() == 0) { s_t[wave_id()][0] = v[0]; s_t[wave_id()][1] = v[1]; }
        __syncthreads();
        v[0] = (s_t[0][0] + s_t[1][0]) + (s_t[2][0] + s_t[3][0]);
        v[1] = (s_t[0][1] + s_t[1][1]) + (s_t[2][1] + s_t[3][1]);
    }
}
// the block's normalised weights w_i = q_i / S of the lane's ITEMS particles (0 beyond the block), as a view of the block has them: K from the
// block's particle count, maximum and flags of the block (safe_softmax, utils.jl:119-126), q = 1 for an all -Inf block.  Returns the flags.
template <int TEAM, int ITEMS>
__device__ __forceinline__ int block_norm_weights(const double* __restrict__ lw, int64_t b0, int cnt, int tl, double* s_m, int* s_f, uint64_t (*s_x)[4],
                                                  double (&w)[ITEMS])
{
    const int K = fix_K(cnt);
    double lwv[ITEMS];
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) { const int i = ITEMS * tl + k; lwv[k] = i < cnt ? lw[b0 + i] : -__builtin_huge_val(); }
    double m; int f;
    team_max_flags<TEAM, ITEMS>(lwv, tl, cnt, s_m, s_f, m, f);
    uint64_t q[ITEMS], S = 0;
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) { q[k] = ITEMS * tl + k < cnt ? ((f & FLAG_ALL_NEGINF) ? 1ull : exp_fix(lwv[k] - m, K)) : 0ull; S += q[k]; }
    S = wave_sum_u64(S);
    if (TEAM == BLOCK) {
        __syncthreads();
        if (lane_id() == 0) s_x[wave_id()][0] = S;
        __syncthreads();
        S = 0;
#pragma unroll
        for (int wv = 0; wv < NWAVES; ++wv) S += s_x[wv][0];
    }
    const double Sd = (double)S;
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) w[k] = (double)q[k] / Sd;
    return f;
}
// mean_out / var_out: [nblocks][W]; a block with NaN / +Inf weights gets NaN everywhere.  want_var = 0: var_out is not touched
template <int W, int TEAM, int ITEMS>
__global__ __launch_bounds__(BLOCK) void k_block_moments(const double* __restrict__ rows, const double* __restrict__ lw, int64_t n, int64_t nb, int64_t nblocks,
                                                         int want_var, double* __restrict__ mean_out, double* __restrict__ var_out)
{
    constexpr int TEAMS = BLOCK / TEAM;
    static_assert(TEAM == WAVE || TEAM == BLOCK, "a wave or the workgroup");
    static_assert(W % 2 == 0, "rows are read as 16-byte column pairs");
    __shared__ double s_m[NWAVES];
    __shared__ int s_f[NWAVES];
    __shared__ uint64_t s_x[NWAVES][4];
    __shared__ double s_t[NWAVES][2];
    const int tm = (int)threadIdx.x / TEAM, tl = (int)threadIdx.x % TEAM;
    const int64_t blk = (int64_t)blockIdx.x * TEAMS + tm;
    if (TEAM != BLOCK && blk >= nblocks) return;                   // (an idle wave: the wave-team path has no workgroup barrier)
    const int64_t b0 = blk * nb;
    const int cnt = (int)(n - b0 < nb ? n - b0 : nb);
    double w[ITEMS];
    const int f = block_norm_weights<TEAM, ITEMS>(lw, b0, cnt, tl, s_m, s_f, s_x, w);
    if (f & (FLAG_NAN | FLAG_POSINF)) {                            // (team-uniform)
        for (int c = tl; c < W; c += TEAM) { mean_out[blk * W + c] = __builtin_nan(""); if (want_var) var_out[blk * W + c] = __builtin_nan(""); }
        return;
    }
#pragma unroll 1
    for (int c2 = 0; c2 < W / 2; ++c2) {
        double2 v[ITEMS];
        double t0[ITEMS], t1[ITEMS];
#pragma unroll
        for (int k = 0; k < ITEMS; ++k) {
            const int i = ITEMS * tl + k;
            const bool in = i < cnt;
            v[k] = in ? reinterpret_cast<const double2*>(rows + (b0 + i) * W)[c2] : double2{0.0, 0.0};
            t0[k] = in ? w[k] * v[k].x : 0.0;
            t1[k] = in ? w[k] * v[k].y : 0.0;
        }
        double mu[2] = {lane_tree<ITEMS>(t0), lane_tree<ITEMS>(t1)};
        team_tree2<TEAM>(mu, s_t);
        if (tl == 0) { mean_out[blk * W + 2 * c2] = mu[0]; mean_out[blk * W + 2 * c2 + 1] = mu[1]; }
        if (want_var) {                                            // (grid-uniform)
#pragma unroll
            for (int k = 0; k < ITEMS; ++k) {
                const bool in = ITEMS * tl + k < cnt;
                double d0 = v[k].x - mu[0], d1 = v[k].y - mu[1];
                d0 = d0 * d0; d1 = d1 * d1;
                t0[k] = in ? w[k] * d0 : 0.0;
                t1[k] = in ? w[k] * d1 : 0.0;
            }
            double s2[2] = {lane_tree<ITEMS>(t0), lane_tree<ITEMS>(t1)};
            team_tree2<TEAM>(s2, s_t);
            if (tl == 0) { var_out[blk * W + 2 * c2] = s2[0]; var_out[blk * W + 2 * c2 + 1] = s2[1]; }
        }
    }
}
// proportionmap of one block: out[blk][j] = sum of the weights w of the lane's values x that equal mv.v[j], j < mv.n
constexpr int BLK_MATCH_MAX = 16;
struct BlockMatch { double v[BLK_MATCH_MAX]; int n; };
template <int TEAM, int ITEMS>
__device__ __forceinline__ void block_match_pass(const double (&w)[ITEMS], const double (&x)[ITEMS], int cnt, int tl, const BlockMatch& mv,
                                                 double* __restrict__ out, int64_t blk, double (*s_t)[2])
{
#pragma unroll 1
    for (int j = 0; j < mv.n; j += 2) {                            // two match values per pass (mv.v is padded to an even count)
        const double a0 = mv.v[j], a1 = mv.v[j + 1];
        double t0[ITEMS], t1[ITEMS];
#pragma unroll
        for (int k = 0; k < ITEMS; ++k) {
            const bool in = ITEMS * tl + k < cnt;
            t0[k] = in ? w[k] * (x[k] == a0 ? 1.0 : 0.0) : 0.0;
            t1[k] = in ? w[k] * (x[k] == a1 ? 1.0 : 0.0) : 0.0;
        }
        double p[2] = {lane_tree<ITEMS>(t0), lane_tree<ITEMS>(t1)};
        team_tree2<TEAM>(p, s_t);
        if (tl == 0) { out[blk * mv.n + j] = p[0]; if (j + 1 < mv.n) out[blk * mv.n + j + 1] = p[1]; }
    }
}
// proportionmap: out[blk][j] = sum of the normalised weights of block blk's particles whose `col` equals v[j], j < n  (statistics.jl:91-101)
template <int TEAM, int ITEMS>
__global__ __launch_bounds__(BLOCK) void k_block_proportion(const double* __restrict__ rows, int W, int col, const double* __restrict__ lw, int64_t n, int64_t nb,
                                                            int64_t nblocks, BlockMatch mv, double* __restrict__ out)
{
    constexpr int TEAMS = BLOCK / TEAM;
    static_assert(TEAM == WAVE || TEAM == BLOCK, "a wave or the workgroup");
    __shared__ double s_m[NWAVES];
    __shared__ int s_f[NWAVES];
    __shared__ uint64_t s_x[NWAVES][4];
    __shared__ double s_t[NWAVES][2];
    const int tm = (int)threadIdx.x / TEAM, tl = (int)threadIdx.x % TEAM;
    const int64_t blk = (int64_t)blockIdx.x * TEAMS + tm;
    if (TEAM != BLOCK && blk >= nblocks) return;
    const int64_t b0 = blk * nb;
    const int cnt = (int)(n - b0 < nb ? n - b0 : nb);
    double w[ITEMS];
    const int f = block_norm_weights<TEAM, ITEMS>(lw, b0, cnt, tl, s_m, s_f, s_x, w);
    if (f & (FLAG_NAN | FLAG_POSINF)) {
        for (int j = tl; j < mv.n; j += TEAM) out[blk * mv.n + j] = __builtin_nan("");
        return;
    }
    double x[ITEMS];
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) { const int i = ITEMS * tl + k; x[k] = i < cnt ? rows[(b0 + i) * W + col] : 0.0; }
    block_match_pass<TEAM, ITEMS>(w, x, cnt, tl, mv, out, blk, s_t);
}

// ----------------------------------------------------------------------------- per-block estimates of a PAST choice: the trajectory store, block by block
// for b in blocks; mean(state[b], t => addr); var(state[b], t => addr); proportionmap(state[b], t => addr); end -- a Gen trace is persistent and a
// sub-state is a slice of the traces (statistics.jl:13-14, 48-50, 91-101 with a past address on ParticleFilterSubStates, view.jl:35-48).  ONE launch
// for all blocks and all d latent columns of the store (gpf_history_enable_blocks).  A lane first resolves, for each of its ITEMS particles, the
// particle of step t it descends from: the composed ancestor maps of the steps T, T-1, ..., t+1 in that order (k_hist_column; maps = nullptr entries
// are steps without a resample, n_maps = 0 reads the step's own snapshot), then reads that particle's columns of the step's snapshot hx = [n][D].
// The ancestor may sit in any block (gpf_resample_across_blocks copies whole blocks).  Weights, order of the sums and the NaN rule are those of
// k_block_moments / k_block_proportion -- the same device functions -- so a block's values are bit-identical to those calls on a filter whose rows
// hold the past values.  D may be 1: the snapshot is read by single words.
template <int ITEMS>
__device__ __forceinline__ void block_hist_index(const int32_t* const* __restrict__ maps, int n_maps, int64_t b0, int cnt, int tl, int64_t (&idx)[ITEMS])
{
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) idx[k] = b0 + (ITEMS * tl + k < cnt ? ITEMS * tl + k : 0);        // (beyond the block: the block's first particle, never read)
    for (int s = 0; s < n_maps; ++s) {
        const int32_t* __restrict__ m = maps[s];
        if (!m) continue;                                          // (kernel-uniform)
#pragma unroll
        for (int k = 0; k < ITEMS; ++k) idx[k] = m[idx[k]];
    }
}
// mean_out / var_out: [nblocks][D]; a block with NaN / +Inf weights gets NaN everywhere.  want_var = 0: var_out is not touched
template <int D, int TEAM, int ITEMS>
__global__ __launch_bounds__(BLOCK) void k_block_hist_moments(const int32_t* const* __restrict__ maps, int n_maps, const double* __restrict__ hx,
                                                              const double* __restrict__ lw, int64_t n, int64_t nb, int64_t nblocks, int want_var,
                                                              double* __restrict__ mean_out, double* __restrict__ var_out)
{
    constexpr int TEAMS = BLOCK / TEAM;
    static_assert(TEAM == WAVE || TEAM == BLOCK, "a wave or the workgroup");
    static_assert(D == 1 || D % 2 == 0, "the latent columns go through the tree two at a time");
    __shared__ double s_m[NWAVES];
    __shared__ int s_f[NWAVES];
    __shared__ uint64_t s_x[NWAVES][4];
    __shared__ double s_t[NWAVES][2];
    const int tm = (int)threadIdx.x / TEAM, tl = (int)threadIdx.x % TEAM;
    const int64_t blk = (int64_t)blockIdx.x * TEAMS + tm;
    if (TEAM != BLOCK && blk >= nblocks) return;                   // (an idle wave: the wave-team path has no workgroup barrier)
    const int64_t b0 = blk * nb;
    const int cnt = (int)(n - b0 < nb ? n - b0 : nb);
    double w[ITEMS];
    const int f = block_norm_weights<TEAM, ITEMS>(lw, b0, cnt, tl, s_m, s_f, s_x, w);
    if (f & (FLAG_NAN | FLAG_POSINF)) {                            // (team-uniform)
        for (int c = tl; c < D; c += TEAM) { mean_out[blk * D + c] = __builtin_nan(""); if (want_var) var_out[blk * D + c] = __builtin_nan(""); }
        return;
    }
    int64_t idx[ITEMS];
    block_hist_index<ITEMS>(maps, n_maps, b0, cnt, tl, idx);
    constexpr bool PAIR = D > 1;                                   // (D = 1: the tree's second value only ever adds +0.0)
#pragma unroll 1
    for (int c = 0; c < D; c += 2) {
        double x0[ITEMS], x1[ITEMS], t0[ITEMS], t1[ITEMS];
#pragma unroll
        for (int k = 0; k < ITEMS; ++k) {
            const bool in = ITEMS * tl + k < cnt;
            x0[k] = in ? hx[idx[k] * D + c] : 0.0;
            x1[k] = in && PAIR ? hx[idx[k] * D + c + (PAIR ? 1 : 0)] : 0.0;
            t0[k] = in ? w[k] * x0[k] : 0.0;
            t1[k] = in ? w[k] * x1[k] : 0.0;
        }
        double mu[2] = {lane_tree<ITEMS>(t0), lane_tree<ITEMS>(t1)};
        team_tree2<TEAM>(mu, s_t);
        if (tl == 0) { mean_out[blk * D + c] = mu[0]; if (PAIR) mean_out[blk * D + c + 1] = mu[1]; }
        if (want_var) {                                            // (grid-uniform)
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
            if (tl == 0) { var_out[blk * D + c] = s2[0]; if (PAIR) var_out[blk * D + c + 1] = s2[1]; }
        }
    }
}
// out[blk][j] = sum of the normalised weights of block blk's particles whose past choice (column col of the snapshot hx = [n][d]) equals v[j]
template <int TEAM, int ITEMS>
__global__ __launch_bounds__(BLOCK) void k_block_hist_proportion(const int32_t* const* __restrict__ maps, int n_maps, const double* __restrict__ hx, int d, int col,
                                                                 const double* __restrict__ lw, int64_t n, int64_t nb, int64_t nblocks, BlockMatch mv,
                                                                 double* __restrict__ out)
{
    constexpr int TEAMS = BLOCK / TEAM;
    static_assert(TEAM == WAVE || TEAM == BLOCK, "a wave or the workgroup");
    __shared__ double s_m[NWAVES];
    __shared__ int s_f[NWAVES];
    __shared__ uint64_t s_x[NWAVES][4];
    __shared__ double s_t[NWAVES][2];
    const int tm = (int)threadIdx.x / TEAM, tl = (int)threadIdx.x % TEAM;
    const int64_t blk = (int64_t)blockIdx.x * TEAMS + tm;
    if (TEAM != BLOCK && blk >= nblocks) return;
    const int64_t b0 = blk * nb;
    const int cnt = (int)(n - b0 < nb ? n - b0 : nb);
    double w[ITEMS];
    const int f = block_norm_weights<TEAM, ITEMS>(lw, b0, cnt, tl, s_m, s_f, s_x, w);
    if (f & (FLAG_NAN | FLAG_POSINF)) {
        for (int j = tl; j < mv.n; j += TEAM) out[blk * mv.n + j] = __builtin_nan("");
        return;
    }
    int64_t idx[ITEMS];
    block_hist_index<ITEMS>(maps, n_maps, b0, cnt, tl, idx);
    double x[ITEMS];
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) x[k] = ITEMS * tl + k < cnt ? hx[idx[k] * d + col] : 0.0;
    block_match_pass<TEAM, ITEMS>(w, x, cnt, tl, mv, out, blk, s_t);
}

// ----------------------------------------------------------------------------- whole trajectories per block: the ancestral paths of the store
// for b in blocks; sample_unweighted_traces(state[b], n_samples); end -- a draw from a sub-state is a persistent trace, i.e. a whole path x_1:T of
// the block (src/utils.jl:7,189-194 on a ParticleFilterSubState, src/view.jl:35-48).  ONE launch for all blocks (gpf.h gpf_block_sample_trajectories):
//   weights   the block's fixed-point weights and their inclusive CDF in LDS, exactly as k_block_resample builds them (K from the block's particle
//             count, safe_softmax's maximum and flags, q = 1 for an all -Inf block);
//   draws     draw j of block b reads resample slot b n_samples + j of the call's epoch: a = upper_bound(cdf, mulhi64(U, S)); the draws are dealt to the
//             team's lanes as j = tl, tl + TEAM, ..., so n_samples may exceed the team;
//   walk      every lane follows ITS draw back through the composed ancestor maps: maps[q] (q the 0-based step, nullptr = no resample in that step:
//             kernel-uniform) leads from the final order of step q to that of step q - 1.  On the way down it reads, at every step q in [lo0, hi0],
//             the D latent columns of snapshot hx[q] at the particle it stands on.  A chain of T dependent 4-byte loads per draw: the launch is fast
//             when many draws are in flight, not through anything a lane does.
//   output    traj = [nblocks][n_samples][hi0 - lo0 + 1][D], the layout the caller receives: a lane fills the contiguous run of its own draw, one
//             16-byte piece (D = 1: one word) per step and pair of columns, from the last step down -- every 128-byte line is written by one lane in
//             consecutive iterations and merges in L2; the reads of the walk are one line per lane and step whatever the layout.  idx = [nblocks]
//             [n_samples], 1-based inside the block.  Either may be null.
// A block with NaN / +Inf log-weights: idx 0, NaN paths.  Teams as in k_block_hist_moments.
template <int D, int TEAM, int ITEMS>
__global__ __launch_bounds__(BLOCK) void k_block_sample_traj(const int32_t* const* __restrict__ maps, const double* const* __restrict__ hx, int T, int lo0, int hi0,
                                                             const double* __restrict__ lw, int64_t n, int64_t nb, int64_t nblocks, int n_samples,
                                                             uint64_t seed, uint32_t epoch, double* __restrict__ traj, int64_t* __restrict__ idx_out)
{
    constexpr int TEAMS = BLOCK / TEAM, CAP = TEAM * ITEMS;
    static_assert(TEAM == WAVE || TEAM == BLOCK, "a wave or the workgroup");
    static_assert(D == 1 || D == 2 || D == 4, "the latent columns are moved as words or 16-byte pairs");
    __shared__ uint64_t s_cdf_[BLOCK * ITEMS];
    __shared__ uint64_t s_x[NWAVES][4];
    __shared__ double s_m[NWAVES];
    __shared__ int s_f[NWAVES];
    const int tm = (int)threadIdx.x / TEAM, tl = (int)threadIdx.x % TEAM;
    const int64_t blk = (int64_t)blockIdx.x * TEAMS + tm;
    if (TEAM != BLOCK && blk >= nblocks) return;                   // (an idle wave: the wave-team path has no workgroup barrier)
    uint64_t* const s_cdf = s_cdf_ + tm * CAP;
    const int64_t b0 = blk * nb;
    const int cnt = (int)(n - b0 < nb ? n - b0 : nb);
    const int K = fix_K(cnt);
    const int n_steps = hi0 - lo0 + 1;
    double lwv[ITEMS];
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) { const int i = ITEMS * tl + k; lwv[k] = i < cnt ? lw[b0 + i] : -__builtin_huge_val(); }
    double m; int f;
    team_max_flags<TEAM, ITEMS>(lwv, tl, cnt, s_m, s_f, m, f);
    uint64_t q[ITEMS];
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) q[k] = ITEMS * tl + k < cnt ? ((f & FLAG_ALL_NEGINF) ? 1ull : exp_fix(lwv[k] - m, K)) : 0ull;
    const uint64_t S = team_scan_incl<TEAM, ITEMS>(q, s_x);
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) s_cdf[ITEMS * tl + k] = q[k];
    team_sync<TEAM>();
    const bool bad = (f & (FLAG_NAN | FLAG_POSINF)) != 0;          // (team-uniform)
    for (int j = tl; j < n_samples; j += TEAM) {
        const int64_t draw = blk * n_samples + j;                  // < 2^31 (checked by the host): the draw's resample slot
        int a = -1;
        if (!bad) a = lds_upper_bound(s_cdf, cnt, mulhi64(resample_u64(seed, (uint32_t)draw, epoch), S));
        if (idx_out) idx_out[draw] = (int64_t)a + 1;
        if (!traj) continue;
        double* const out = traj + draw * n_steps * D;
        if (bad) {
            for (int t = 0; t < n_steps * D; ++t) out[t] = __builtin_nan("");
            continue;
        }
        int64_t p = b0 + a;
        for (int s = T - 1; s >= lo0; --s) {
            if (s <= hi0) {
                const double* __restrict__ x = hx[s] + p * D;
                double* const o = out + (s - lo0) * D;
                if constexpr (D == 1) o[0] = x[0];
                else {
#pragma unroll
                    for (int c = 0; c < D / 2; ++c) reinterpret_cast<double2*>(o)[c] = reinterpret_cast<const double2*>(x)[c];
                }
            }
            if (s > lo0) { const int32_t* __restrict__ g = maps[s]; if (g) p = g[p]; }      // (kernel-uniform)
        }
    }
}

// ----------------------------------------------------------------------------- resampling ACROSS blocks: the block-granular gather
// gpf_resample_across_blocks (gpf.h): every block is one "super-particle" with the log-weight L[b] = log_ml_estimate(state[b]); a planner filter
// of nblocks particles resampled them (the reference's resampler, src/resample.jl:19-175, one level up) and left the source block A[b] of every
// destination block on the device.  This kernel copies whole filters: destination particle p = b nb + i takes the row, the log-weight and the
// per-block rows of particle A[b] nb + i,
//     lw'[p] = lw[A[b] nb + i] + delta_a,  delta_a = M - L[a]  (0 where L[a] = -Inf),  parents'[p] = A[b] nb + i + 1,
// so the weights INSIDE a block are kept (its inner filter carries on) and only its total mass becomes the average mass M.
// A block's rows are one contiguous, 16-byte aligned run of nb W doubles: the copy is a stream of 16-byte pieces with a block-granular source
// offset.  The grid is sized by BYTES, not by blocks -- one workgroup per chunk of BG_PIECES pieces of the destination (16 KB of rows, and
// the log-weights and parents of the same particles), grid-striding beyond the launch's workgroups -- so 10^4 blocks of 100 particles and 8
// blocks of 10^5 fill the machine alike, and there is no LDS limit on nb.  A lane issues all its loads before its stores.  The per-block
// parameter and observation rows (a few hundred bytes per block) ride in the same launch.  Traffic: 2 (8 W + 16) n bytes incl. the ancestor words.
constexpr int BG_PIECES = 1024;                    // 16-byte pieces of rows per chunk
struct BlockGatherArgs {
    const double* rows_in; double* rows_out;       // the ping-pong row buffers
    const double* lw_in; double* lw_out;           // log-weights: read at the source, written to a second array (the host swaps them)
    int32_t* anc_out;                              // state.parents (0-based here)
    const int32_t* A;                              // [nblocks] source block of every destination block (the planner's ancestors)
    const double* L;                               // [nblocks] block log-weights
    double M;                                      // log_ml_estimate(planner) = logsumexp(L) - log(nblocks)
    const double* par_in; double* par_out;         // [nblocks][MAX_PARAMS] or null
    const double* obs_in; double* obs_out;         // [nblocks][MAX_OBS] or null
    int64_t n; int32_t nb, nblocks;
};
template <int W>
__global__ __launch_bounds__(BLOCK) void k_block_gather(BlockGatherArgs a)
{
    constexpr int PW = W / 2;                      // pieces per row
    constexpr int CP = BG_PIECES / PW;             // particles per chunk
    constexpr int PER = BG_PIECES / BLOCK;         // pieces per lane and chunk
    constexpr int PPER = CP / BLOCK;               // particles per lane and chunk
    static_assert(CP % BLOCK == 0 && PPER >= 1, "a chunk is a whole number of particles per lane");
    const uint32_t nb = (uint32_t)a.nb;
    const int32_t last = a.nblocks - 1;
    // (the planner's search clamps its ancestors to [0, nblocks); the clamp here costs nothing and keeps every read inside the buffers)
    auto src_block = [&](uint32_t b) { const int32_t s = a.A[b]; return (uint32_t)(s < 0 ? 0 : (s > last ? last : s)); };
    const int64_t gt = (int64_t)blockIdx.x * BLOCK + threadIdx.x, gs = (int64_t)gridDim.x * BLOCK;
    if (a.par_in)
        for (int64_t i = gt; i < (int64_t)a.nblocks * MAX_PARAMS; i += gs) {
            const uint32_t b = (uint32_t)i / (uint32_t)MAX_PARAMS, k = (uint32_t)i - b * MAX_PARAMS;
            a.par_out[i] = a.par_in[(size_t)src_block(b) * MAX_PARAMS + k];
        }
    if (a.obs_in)
        for (int64_t i = gt; i < (int64_t)a.nblocks * MAX_OBS; i += gs) {
            const uint32_t b = (uint32_t)i / (uint32_t)MAX_OBS, k = (uint32_t)i - b * MAX_OBS;
            a.obs_out[i] = a.obs_in[(size_t)src_block(b) * MAX_OBS + k];
        }
    typedef double piece_t __attribute__((ext_vector_type(2)));      // (a native vector: an array of them stays in registers)
    const piece_t* __restrict__ in2 = reinterpret_cast<const piece_t*>(a.rows_in);
    piece_t* __restrict__ out2 = reinterpret_cast<piece_t*>(a.rows_out);
    const int64_t nchunks = (a.n + CP - 1) / CP;
    for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const int64_t p0 = c * CP;
        piece_t v[PER];
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const uint32_t e = (uint32_t)(k * BLOCK) + threadIdx.x;
            const int64_t p = p0 + e / PW;
            v[k] = piece_t{0.0, 0.0};
            if (p < a.n) {
                const uint32_t b = (uint32_t)p / nb, i = (uint32_t)p - b * nb;
                v[k] = in2[((size_t)src_block(b) * nb + i) * PW + e % PW];
            }
        }
        double w[PPER]; int32_t s[PPER];
#pragma unroll
        for (int k = 0; k < PPER; ++k) {
            const int64_t p = p0 + k * BLOCK + threadIdx.x;
            w[k] = 0.0; s[k] = 0;
            if (p < a.n) {
                const uint32_t b = (uint32_t)p / nb, i = (uint32_t)p - b * nb, sb = src_block(b);
                const double Ls = a.L[sb];
                const double delta = Ls == -__builtin_huge_val() ? 0.0 : a.M - Ls;
                s[k] = (int32_t)(sb * nb + i);
                w[k] = a.lw_in[s[k]] + delta;
            }
        }
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const uint32_t e = (uint32_t)(k * BLOCK) + threadIdx.x;
            if (p0 + e / PW < a.n) out2[(size_t)p0 * PW + e] = v[k];
        }
#pragma unroll
        for (int k = 0; k < PPER; ++k) {
            const int64_t p = p0 + k * BLOCK + threadIdx.x;
            if (p < a.n) { a.lw_out[p] = w[k]; a.anc_out[p] = s[k]; }
        }
    }
}

// the end of a staging kernel: the last workgroup to arrive publishes `ticket` to pinned memory; the host may then refill that staging buffer.  The
// ticket says "the staging buffer has been READ": every load of a workgroup has returned -- its value went into a store that has been issued --
// before the barrier; nothing the host reads is published, so no fence: an agent / system release is an L2 write-back
__device__ __forceinline__ void stage_ticket(unsigned int* counter, int64_t* host_done, int64_t ticket)
{
    __syncthreads();
    if (threadIdx.x == 0) {
        if (__hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1) {
            __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(host_done, ticket, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}
// the blocks' observation vectors from a pinned host buffer into device memory, by a KERNEL (coalesced reads over PCIe) rather than a
// hipMemcpyAsync: the copy stays on the compute queue (an SDMA copy costs a cross-queue dependency of ~10-20 us in front of the step
// kernel that reads it).  Ends with stage_ticket.
static __global__ __launch_bounds__(BLOCK) void k_stage_obs(const double* __restrict__ src_host, double* __restrict__ dst, int64_t n_words,
                                                     unsigned int* counter, int64_t* host_done, int64_t ticket)
{
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n_words; i += (int64_t)gridDim.x * BLOCK) dst[i] = src_host[i];
    stage_ticket(counter, host_done, ticket);
}

// k_stage_obs with the reference rows of a pinned step behind the observations in the SAME staging buffer: src_host = [n_obs_words | n_ref_words],
// the first part to dst_obs, the second to dst_ref -- one launch, one ticket
static __global__ __launch_bounds__(BLOCK) void k_stage_obs_ref(const double* __restrict__ src_host, double* __restrict__ dst_obs, int64_t n_obs_words,
                                                         double* __restrict__ dst_ref, int64_t n_ref_words,
                                                         unsigned int* counter, int64_t* host_done, int64_t ticket)
{
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n_obs_words + n_ref_words; i += (int64_t)gridDim.x * BLOCK) {
        const double v = src_host[i];
        if (i < n_obs_words) dst_obs[i] = v; else dst_ref[i - n_obs_words] = v;
    }
    stage_ticket(counter, host_done, ticket);
}

} // namespace gpf
