// K11i: a whole series per block in one launch, blocks of up to 8192 particles  (part of gpf_kernels.hpp; include that header, not this file)
#pragma once

namespace gpf {
// ----------------------------------------------------------------------------- the filter loop of a few large filters, block by block
// gpf_run_blocks_wide (gpf.h): k_block_run's step -- gate, optional bitonic order, CDF(s), search, default-proposal propagate, summary
// (gpf_k_block_run.hpp, whose comment says what each of them restates) -- for blocks of 2049 .. 8192 particles, which the loop of calls runs through
// sub-state views with the full-size kernels.  One workgroup of WIDE = 512 threads (8 waves) runs all n_steps iterations of one block.
// Team shape: 1024 threads leave a wave 128 VGPRs, and at that budget all fifteen instantiations spill (96 .. 304 bytes of scratch per lane: the
// model's sampler and density alone take most of it); at 512 threads they need 158 .. 204 VGPRs and no scratch (profiles/block_run_wide.md).
//
// Why this is not k_block_run with more ITEMS.  k_block_run keeps a block in REGISTERS across the phases of a step: ITEMS consecutive fixed-point
// weights per lane, their scans, the residual counts (q[], c[], r[]: 48 VGPRs at ITEMS = 8 before the model's sampler).  At 8192 particles that is
// 16 items per lane of 512 threads -- 96 VGPRs of block state beside a sampler that takes 150 and more -- or 32 per lane of 256.  Here the block's
// state lives in LDS -- gfx950 has 160 kB per CU -- and a lane holds a value only while it works on it:
//   s_q    [cap] u64   the fixed-point weights, written ONCE per step by the summary; the resample turns them into the CDF that is sampled IN PLACE
//                      (residual: into the residual weights, then their CDF)
//   s_aux  [cap] u64   residual: the copy counts, then their CDF; stratified with sort_particles: the sort keys
//   s_idx  [cap] u16   stratified with sort_particles: the order
// cap = wide_cap(block size), the network's size; dynamic LDS of 8 | 16 | 18 bytes x cap by method (64 | 128 | 144 kB at 8192), beside 1.4 kB static.
// Lanes stride over the block (slot j = tl, tl + 512, ...): the summary, the residual split and the slot loop touch element j from the SAME lane, LDS
// and global accesses of a wave are consecutive, and a ragged or small last block simply leaves the upper lanes idle.
// Scans (wide_scan): wave w owns the contiguous chunk [w c, (w + 1) c), c = 64 ceil(cnt / 512); it scans its chunk strip by strip of 64 elements with
// wave_scan_u64, carrying the running total, and leaves the chunk's total in LDS; the 8 totals give every wave its offset, which it adds to its own
// chunk.  Two barriers per scan whatever the size; the residual's two CDFs share them.  All of it exact integer arithmetic: the layout and the order
// of the sums cannot show in a result.
// The weight summary: (m, f) are a maximum and an OR, so the lanes' stride instead of k_block_stats' consecutive items changes no bit; q = exp_fix of
// the same argument; S and Q exact sums.  S of the resample IS the summary's S (k_block_run re-scans to get it; the sorted order permutes the same
// terms).
//
// Arithmetic for cnt <= BLK_WIDE_MAX = 2^13 (gpf_k_block.hpp derives these for 2^11):
//   K = fix_K(cnt) = min(52, 62 - ceil_log2(cnt)), so q <= 2^K and S <= cnt 2^K <= 2^62 in a u64 for every cnt (49 bits of weight at 8192).
//   Q = sum q^2 <= cnt 2^(2 K): 2^114 at cnt = 1024 (K = 52), 2^111 at 8192 (K = 49), in a u128.  A lane holds ceil(cnt / 512) terms, 2^105 (two terms
//       at K = 52) .. 2^102 (sixteen at K = 49): its high word is <= 2^41.  The three limbs summed over 512 lanes are < 2^41, < 2^41 and <= 2^50.
//   residual: n q = cnt q <= 2^62.  The quotient (n q) div S <= cnt <= 2^13; the double estimate (double)(n q) / (double)S carries three roundings of
//       2^-53 relative each, an absolute error < 2^13 3 2^-53 < 2^-38, so its truncation is the quotient or one off on either side: the same two exact
//       corrections.  cq S <= n q + S <= 2^63 before the first correction.  residual_shift keeps cnt (S >> sh) <= 2^62 for any cnt by its definition.
//   stratified: the strata bound floor(j S / cnt) = j sB + floor(j srem / cnt) with j + 1 <= 2^13 and srem < cnt <= 2^13: the products stay < 2^26,
//       32-bit divisions as before.
//   order: 16-bit indices < 8192; the network pads to p2 <= 8192 = cap with keys ~0, which sort behind every weight.
// Synchronisation: __syncthreads between phases; hipcc puts s_waitcnt vmcnt(0) lgkmcnt(0) in front of each, and the waves of a workgroup share their
// CU's L1, so rows and log-weights stored before the barrier are what loads behind it return (run_sync<BLOCK>'s argument, gpf_k_block_run.hpp).  No spin
// waits, nothing between workgroups; every loop is bounded by n_steps, cnt or the network's size.  Every branch around a barrier is team-uniform: go,
// the method and the sizes derive from kernel arguments and from sums every lane reads from the same LDS words.
// A block per workgroup and a workgroup per CU (the LDS): fewer than 256 blocks leave CUs idle -- a block spread over several workgroups is not built.
constexpr int BLK_WIDE_MAX = 8192;                 // particles per block
constexpr int WIDE = 512;                          // threads of the team
constexpr int WIDE_WAVES = WIDE / WAVE, WIDE_ITEMS = BLK_WIDE_MAX / WIDE;
// the capacity of the LDS arrays for blocks of nb particles: the bitonic network's size, at least a strip
GPF_HD int wide_cap(int64_t nb) { int c = WAVE; while (c < nb) c <<= 1; return c; }
GPF_HD size_t wide_lds_bytes(int method, int64_t nb) { return (size_t)wide_cap(nb) * (method == 0 ? 8u : method == 1 ? 16u : 18u); }

// in-place inclusive scan of a[0, cnt) -- TWO: and of b[0, cnt) -- over the team; the totals in ta, tb.  The caller's barrier stands in front (the
// elements come from other lanes); a barrier closes it.  s_t: [WIDE_WAVES][2] words of LDS
template <bool TWO>
__device__ __forceinline__ void wide_scan(uint64_t* a, uint64_t* b, int cnt, int tl, uint64_t (*s_t)[2], uint64_t& ta, uint64_t& tb)
{
    const int wv = tl >> 6, ln = tl & (WAVE - 1);
    const int chunk = ((cnt + WIDE - 1) / WIDE) * WAVE;            // (the waves' chunks cover cnt)
    const int lo = wv * chunk, hi = lo + chunk < cnt ? lo + chunk : cnt;
    uint64_t ca = 0, cb = 0;
    for (int base = lo; base < hi; base += WAVE) {                 // (wave-uniform bounds: the shuffles see all 64 lanes)
        const int i = base + ln;
        const uint64_t va = wave_scan_u64(i < hi ? a[i] : 0ull) + ca;
        if (i < hi) a[i] = va;
        ca = shfl_u64(va, WAVE - 1);
        if (TWO) {
            const uint64_t vb = wave_scan_u64(i < hi ? b[i] : 0ull) + cb;
            if (i < hi) b[i] = vb;
            cb = shfl_u64(vb, WAVE - 1);
        }
    }
    if (ln == 0) { s_t[wv][0] = ca; s_t[wv][1] = cb; }
    __syncthreads();
    uint64_t pa = 0, pb = 0;
    ta = 0; tb = 0;
#pragma unroll
    for (int w = 0; w < WIDE_WAVES; ++w) {
        const uint64_t xa = s_t[w][0], xb = TWO ? s_t[w][1] : 0ull;
        if (w < wv) { pa += xa; pb += xb; }
        ta += xa; tb += xb;
    }
    for (int i = lo + ln; i < hi; i += WAVE) {                     // (the lane that wrote a[i] above)
        a[i] += pa;
        if (TWO) b[i] += pb;
    }
    __syncthreads();
}
// what a step closes and the next one opens with: maximum, flags, the fixed-point weights (into s_q), their sum and the ESS of the block's current
// log-weights.  Two barriers; the caller's barrier stands in front (lw, and the last readers of s_q)
__device__ __forceinline__ void wide_summary(const double* lw, int cnt, int K, int tl, uint64_t* s_q, double* s_m, int* s_f, uint64_t (*s_x)[4],
                                             double& m_out, int& f_out, uint64_t& S, double& ess)
{
    const int wv = tl >> 6, ln = tl & (WAVE - 1);
    double lwv[WIDE_ITEMS];
    double m = -__builtin_huge_val(); int f = 0;
#pragma unroll
    for (int k = 0; k < WIDE_ITEMS; ++k) {
        const int j = tl + WIDE * k;
        lwv[k] = j < cnt ? lw[j] : -__builtin_huge_val();
        if (j < cnt) { const double x = lwv[k]; if (x != x) f |= FLAG_NAN; else { m = x > m ? x : m; if (x == __builtin_huge_val()) f |= FLAG_POSINF; } }
    }
    m = wave_max_f64(m);
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) f |= __shfl_xor(f, s, WAVE);
    if (ln == 0) { s_m[wv] = m; s_f[wv] = f; }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < WIDE_WAVES; ++w) { m = s_m[w] > m ? s_m[w] : m; f |= s_f[w]; }
    if (!(f & FLAG_NAN) && m == -__builtin_huge_val()) f |= FLAG_ALL_NEGINF;
    unsigned __int128 Q = 0; uint64_t sl = 0;
#pragma unroll
    for (int k = 0; k < WIDE_ITEMS; ++k) {
        const int j = tl + WIDE * k;
        if (j < cnt) {
            const uint64_t q = (f & FLAG_ALL_NEGINF) ? 1ull : exp_fix(lwv[k] - m, K);
            s_q[j] = q;
            Q += (unsigned __int128)q * q; sl += q;
        }
    }
    // 128-bit team sum by limbs: the low word in two 32-bit halves (their carries just add up)
    uint64_t v4[4] = {(uint64_t)Q & 0xffffffffull, (uint64_t)Q >> 32, (uint64_t)(Q >> 64), sl};
#pragma unroll
    for (int c = 0; c < 4; ++c) v4[c] = wave_sum_u64(v4[c]);
    if (ln == 0) { for (int c = 0; c < 4; ++c) s_x[wv][c] = v4[c]; }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 4; ++c) { uint64_t t = 0; for (int w = 0; w < WIDE_WAVES; ++w) t += s_x[w][c]; v4[c] = t; }
    S = v4[3];
    const unsigned __int128 Qt = ((unsigned __int128)v4[2] << 64) + ((unsigned __int128)v4[1] << 32) + v4[0];
    ess = ess_from(S, (uint64_t)(Qt >> 64), (uint64_t)Qt);
    m_out = m; f_out = f;
}
template <int M, int W, int METHOD>                // METHOD 0 multinomial, 1 residual, 2 stratified; W = row_width(Model<M>::D, false)
__global__ __launch_bounds__(WIDE) void k_block_run_wide(RunArgs a)
{
    using Mo = Model<M>;
    constexpr int D = Mo::D;
    static_assert(W >= D && W % 2 == 0, "rows are moved as 16-byte column pairs");
    static_assert(BLK_WIDE_MAX <= 65536 && WIDE_ITEMS * WIDE == BLK_WIDE_MAX, "16-bit order; the summary's items cover the largest block");
    extern __shared__ uint64_t s_wide_dyn[];                       // s_q | s_aux | s_idx, sized by the launch (wide_lds_bytes)
    __shared__ uint64_t s_x[WIDE_WAVES][4];
    __shared__ uint64_t s_t[WIDE_WAVES][2];
    __shared__ double s_m[WIDE_WAVES];
    __shared__ int s_f[WIDE_WAVES];
    const int cap = wide_cap(a.nb);                                // (what the launch sized the dynamic LDS for)
    uint64_t* const s_q = s_wide_dyn;
    uint64_t* const s_aux = s_wide_dyn + (METHOD == 0 ? 0 : cap);
    uint16_t* const s_idx = reinterpret_cast<uint16_t*>(s_wide_dyn + (METHOD == 2 ? 2 * cap : 0));
    const int tl = (int)threadIdx.x;
    const int64_t blk = (int64_t)blockIdx.x;
    const int64_t b0 = blk * a.nb;
    const int cnt = (int)(a.n - b0 < a.nb ? a.n - b0 : a.nb);      // particles of this block
    const int K = fix_K(cnt);
    const double* const P = a.blk_params ? a.blk_params + blk * MAX_PARAMS : a.P;      // (team-uniform)
    const double* const obs_b = a.obs + (a.obs_blocks == 1 ? 0 : (size_t)blk * (size_t)a.n_steps * (size_t)a.n_obs);      // the block's series
    const double lml0 = *a.lml_est;
    double* const lw = a.lw + b0;
    int side = 0, flags_all = 0;
    double m; int f; uint64_t S; double ess;
    wide_summary(lw, cnt, K, tl, s_q, s_m, s_f, s_x, m, f, S, ess);
#pragma unroll 1
    for (int t = 0; t < a.n_steps; ++t) {
        // ================ the resample of step t, epoch E + 2t (k_block_run's statements)
        const uint32_t ep_r = a.epoch + 2u * (uint32_t)t, ep_u = ep_r + 1u;
        const bool gate = a.ess_frac >= 0.0 ? (f == 0 && ess < a.ess_frac * (double)cnt) : true;
        const bool skip = (f & (FLAG_NAN | FLAG_POSINF)) != 0;
        const bool uniform = (f & FLAG_ALL_NEGINF) != 0;
        const bool go = gate && !skip;
        if (tl == 0) a.res_out[(int64_t)t * a.nblocks + blk] = (go ? 1 : 0) | ((gate ? f : 0) << 8);
        flags_all |= gate ? f : 0;
        uint64_t Ctot = 0, Rs = 0;
        if (go) {
            // ---- sort_particles: the bitonic network over (key, index) pairs in s_aux / s_idx, then the weights in sorted order into s_q
            if (METHOD == 2 && a.sorted) {
                int p2 = 2;
                while (p2 < cnt) p2 <<= 1;                         // (<= cap)
                for (int i = tl; i < p2; i += WIDE) { s_aux[i] = i < cnt ? sort_key_desc(lw[i]) : ~0ull; s_idx[i] = (uint16_t)i; }
                __syncthreads();
                for (int size = 2; size <= p2; size <<= 1) {
                    for (int stride = size >> 1; stride >= 1; stride >>= 1) {
                        for (int e = tl; e < p2 / 2; e += WIDE) {
                            const int lo = 2 * e - (e & (stride - 1)), hi = lo + stride;
                            const bool up = (lo & size) == 0;
                            const uint64_t ka = s_aux[lo], kb = s_aux[hi];
                            const uint16_t ia = s_idx[lo], ib = s_idx[hi];
                            const bool gt = ka > kb || (ka == kb && ia > ib);
                            if (gt == up) { s_aux[lo] = kb; s_aux[hi] = ka; s_idx[lo] = ib; s_idx[hi] = ia; }
                        }
                        __syncthreads();
                    }
                }
                for (int i = tl; i < cnt; i += WIDE) s_q[i] = uniform ? 1ull : exp_fix(sort_key_value(s_aux[i]) - m, K);
                __syncthreads();
            }
            // ---- the CDF(s), in place
            if (METHOD == 1) {
                // copies c_i = (N q_i) div S into s_aux, residual weights ((N q_i) mod S) >> sh into s_q (element j by the lane whose summary wrote it)
                const int sh = residual_shift(S, cnt);
                for (int j = tl; j < cnt; j += WIDE) {
                    const uint64_t nq = (uint64_t)cnt * s_q[j];
                    uint64_t cq = (uint64_t)((double)nq / (double)S), prod = cq * S;
                    if (prod > nq) { cq -= 1; prod -= S; }
                    uint64_t rq = nq - prod;
                    if (rq >= S) { cq += 1; rq -= S; }
                    s_aux[j] = cq; s_q[j] = rq >> sh;
                }
                __syncthreads();
                wide_scan<true>(s_aux, s_q, cnt, tl, s_t, Ctot, Rs);
            } else {
                uint64_t tot, none;
                wide_scan<false>(s_q, nullptr, cnt, tl, s_t, tot, none);      // (tot == S)
            }
        }
        // (resample.jl:205-211: every particle of a block that resampled carries the block's average weight)
        const double new_lw = go ? lse_from(m, S, K, f) - log_((double)cnt) : 0.0;
        const uint64_t sB = METHOD == 2 && go ? S / (uint64_t)cnt : 0, srem = METHOD == 2 && go ? S % (uint64_t)cnt : 0;
        // ================ the slots: ancestor (resample), then k_step's default proposal under epoch E + 2t + 1
        double ob[MAX_OBS];                                        // (team-uniform: the block's row of step t, zero-padded)
        {
            const double* const orow = obs_b + (size_t)t * (size_t)a.n_obs;
#pragma unroll
            for (int k = 0; k < MAX_OBS; ++k) ob[k] = k < a.n_obs ? orow[k] : 0.0;
        }
        const double* const rows_in = a.rows[side] + b0 * W;
        double* const rows_out = a.rows[go ? 1 - side : side] + b0 * W;
        for (int j = tl; j < cnt; j += WIDE) {                     // consecutive lanes, consecutive slots: coalesced stores
            const uint32_t slot = (uint32_t)(a.gid0 + b0 + j);
            int anc = j;
            if (go) {
                if (METHOD == 0) anc = lds_upper_bound(s_q, cnt, mulhi64(resample_u64(a.seed, slot, ep_r), S));             // :59
                else if (METHOD == 1) {
                    if ((uint64_t)j < Ctot) anc = lds_upper_bound(s_aux, cnt, (uint64_t)j);                                 // :101 (no draw)
                    else anc = lds_upper_bound(s_q, cnt, mulhi64(resample_u64(a.seed, slot, ep_r), Rs));                    // :113
                } else {
                    const uint64_t jl = (uint64_t)j;                                                               // strata are local to the block
                    const uint64_t L0 = jl * sB + (uint32_t)(jl * srem) / (uint32_t)cnt, L1 = (jl + 1) * sB + (uint32_t)((jl + 1) * srem) / (uint32_t)cnt;
                    anc = lds_upper_bound(s_q, cnt, L0 + mulhi64(resample_u64(a.seed, slot, ep_r), L1 - L0));             // :162-166
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
        __syncthreads();                                           // rows and weights of this step: visible to the team (and s_q / s_aux / s_idx free again)
        // ================ k_block_stats: step t's outputs, step t + 1's gate and weights
        wide_summary(lw, cnt, K, tl, s_q, s_m, s_f, s_x, m, f, S, ess);
        if (tl == 0) {
            a.ess_out[(int64_t)t * a.nblocks + blk] = f ? __builtin_nan("") : ess;                          // (lognorm of invalid weights is NaN)
            a.lml_out[(int64_t)t * a.nblocks + blk] = (lml0 + lse_from(m, S, K, f)) - log_((double)cnt);    // utils.jl:174-178, left to right
        }
    }
    if (tl == 0) a.flags_out[blk] = flags_all << 8;
    if (tl < MAX_OBS)                                              // the block's row of the handle's per-block observations: the last step's
        a.blk_obs[blk * MAX_OBS + tl] = tl < a.n_obs ? obs_b[(size_t)(a.n_steps - 1) * (size_t)a.n_obs + tl] : 0.0;
    if (side)                                                      // (the last step's barrier ordered the rows)
        for (int e = tl; e < cnt * (W / 2); e += WIDE)
            reinterpret_cast<double2*>(a.rows[0] + b0 * W)[e] = reinterpret_cast<const double2*>(a.rows[1] + b0 * W)[e];
}

} // namespace gpf
