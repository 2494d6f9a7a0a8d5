// pf_coalesce! / pf_introduce! (reference src/resize.jl:309-421): a group-by over particle rows, and n fresh trajectories over a
// whole observation history in one launch.  Included by libgpf_aux.hip after gpf_host.hpp (which brings gpf_kernels.hpp).
#pragma once

namespace gpf {
// ----------------------------------------------------------------------------- pf_coalesce! (resize.jl:309-334)
// Open-addressing table of T = 2^k >= 2n slots.  claim[s]: EMPTY, or the index of a member of the group that owns slot s -- it only
// ever moves from EMPTY to a member and then down to smaller members (atomicMin), so whatever value a thread reads names a row with the
// group's key, and after pass 1 it is the group's FIRST member.  gm[2 s] = order-preserving key of the group's maximum weight (max_key),
// gm[2 s + 1] = the exact u64 sum of the members' fixed-point weights exp_fix(w - m, K).  Integer atomics only: bit-reproducible.
constexpr uint32_t COAL_EMPTY = 0xffffffffu;
constexpr int COAL_ITEMS = 8;                              // particles per thread of the tile kernels
constexpr int COAL_TILE = BLOCK * COAL_ITEMS;              // particles per workgroup of passes 2 and 4
constexpr int COAL_ROUNDS = 4;                             // wave-aggregation rounds before the remaining lanes go to the atomics alone

struct CoalArgs {
    const double* rows; const double* lw; int64_t n; uint32_t mask;   // key columns: bit c = column c of the row
    uint32_t* claim; unsigned long long* gm; uint32_t* slot_of; uint64_t tmask;   // slots: T <= 2^32 (n < 2^31), so uint32
    int K;
    unsigned long long* misc;                              // [0] invalid-weight flags, [1] n_new
    uint32_t* tile_cnt; uint32_t* tile_off; int64_t ntiles;
};

template <int W>
__device__ __forceinline__ uint64_t coal_hash(const double (&r)[W], uint32_t mask)
{
    uint64_t h = 0x243f6a8885a308d3ull;
#pragma unroll
    for (int c = 0; c < W; ++c)
        if (mask >> c & 1u) { h = (h ^ d2u(r[c])) * 0x9e3779b97f4a7c15ull; h ^= h >> 29; }
    h = (h ^ (h >> 32)) * 0xd6e8feb86659fd93ull;
    return h ^ (h >> 32);
}
template <int W>
__device__ __forceinline__ bool coal_same(const double* __restrict__ row, const double (&r)[W], uint32_t mask)
{
    bool eq = true;
#pragma unroll
    for (int c = 0; c < W; ++c)
        if (mask >> c & 1u) eq = eq && d2u(row[c]) == d2u(r[c]);          // bitwise: -0.0 != 0.0 (Julia's isequal)
    return eq;
}
// claim[] only moves down and gm[2 s] only up, so a value read without coherence (workgroup scope: may come from this CU's cache, may be
// stale) is an upper / lower bound of the true one: an update it shows to be useless is skipped, any other goes to the atomic.  Without
// this the two-group case spent 3.4 ms in pass 1 on same-address atomics (profiles/coalesce_introduce.md).
__device__ __forceinline__ uint32_t coal_peek(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ unsigned long long coal_peek(const unsigned long long* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void coal_min_max(uint32_t s, uint32_t vi, unsigned long long vk, uint32_t* claim, unsigned long long* gm)
{
    if (vi < coal_peek(claim + s)) atomicMin(&claim[s], vi);
    if (vk > coal_peek(gm + 2 * (int64_t)s)) atomicMax(&gm[2 * (int64_t)s], vk);
}
// Contention (cdna_hip_programming.md Guideline 12): coalescing object_motion by `moving` sends 10^6 updates to two slots.  The lanes of
// a wave that hit the leader's slot are combined first (one atomic per group and wave); after a round whose group is a single lane --
// the keys look distinct -- or after COAL_ROUNDS rounds, every remaining lane issues its own atomics.  Called by whole waves.
__device__ __forceinline__ void coal_first_max(bool act, uint32_t s, uint32_t idx, unsigned long long mk, uint32_t* claim, unsigned long long* gm)
{
    bool pend = act;
    for (int r = 0; r < COAL_ROUNDS; ++r) {
        const unsigned long long pm = __ballot(pend);
        if (pm == 0) return;
        const int leader = __builtin_ctzll(pm);
        const uint32_t ls = (uint32_t)__shfl((int)s, leader, WAVE);
        const bool mine = pend && s == ls;
        const unsigned long long grp = __ballot(mine);
        if (__popcll(grp) == 1) break;
        uint32_t vi = mine ? idx : COAL_EMPTY;
        unsigned long long vk = mine ? mk : 0ull;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const uint32_t oi = (uint32_t)__shfl_xor((int)vi, o, WAVE);
            const unsigned long long ok = shfl_xor_u64(vk, o);
            vi = oi < vi ? oi : vi; vk = ok > vk ? ok : vk;
        }
        if (lane_id() == leader) coal_min_max(ls, vi, vk, claim, gm);
        pend = pend && !mine;
    }
    if (pend) coal_min_max(s, idx, mk, claim, gm);
}
__device__ __forceinline__ void coal_add(bool act, uint32_t s, unsigned long long q, unsigned long long* gm)
{
    bool pend = act;
    for (int r = 0; r < COAL_ROUNDS; ++r) {
        const unsigned long long pm = __ballot(pend);
        if (pm == 0) return;
        const int leader = __builtin_ctzll(pm);
        const uint32_t ls = (uint32_t)__shfl((int)s, leader, WAVE);
        const bool mine = pend && s == ls;
        if (__popcll(__ballot(mine)) == 1) break;
        const unsigned long long v = wave_sum_u64(mine ? q : 0ull);
        if (lane_id() == leader) atomicAdd(&gm[2 * (int64_t)ls + 1], v);
        pend = pend && !mine;
    }
    if (pend) atomicAdd(&gm[2 * (int64_t)s + 1], q);
}

// pass 1: find / claim the group's slot, first member (atomicMin), group maximum (atomicMax); NaN / +Inf weights raise misc[0]
template <int W>
__global__ __launch_bounds__(BLOCK) void k_coal_insert(CoalArgs a)
{
    for (int64_t base = (int64_t)blockIdx.x * BLOCK; base < a.n; base += (int64_t)gridDim.x * BLOCK) {   // whole waves stay in the loop
        const int64_t i = base + threadIdx.x;
        const bool act = i < a.n;
        uint32_t s = 0;
        unsigned long long mk = 0;
        bool bad = false;
        if (act) {
            double r[W];
            const double2* src = reinterpret_cast<const double2*>(a.rows + i * W);
#pragma unroll
            for (int c = 0; c < W / 2; ++c) { const double2 v = src[c]; r[2 * c] = v.x; r[2 * c + 1] = v.y; }
            const double w = a.lw[i];
            bad = w != w || w == __builtin_huge_val();
            mk = bad ? 0ull : max_key(w);
            uint64_t p = coal_hash<W>(r, a.mask) & a.tmask;
            while (true) {                                                  // T >= 2n: an empty slot always exists
                uint32_t c = coal_peek(a.claim + p);                        // (stale EMPTY: the CAS tells; stale member: still a member)
                if (c == COAL_EMPTY) {
                    c = atomicCAS(a.claim + p, COAL_EMPTY, (uint32_t)i);
                    if (c == COAL_EMPTY) break;
                }
                if (coal_same<W>(a.rows + (int64_t)c * W, r, a.mask)) break;
                p = (p + 1) & a.tmask;
            }
            s = (uint32_t)p;
            a.slot_of[i] = s;
        }
        if (__ballot(bad) && lane_id() == 0) atomicOr(a.misc, 1ull);
        coal_first_max(act, s, (uint32_t)i, mk, a.claim, a.gm);
    }
}
// pass 2: the group sums of exp_fix(w - m_g, K); per tile the number of first members (claim[slot] == i)
static __global__ __launch_bounds__(BLOCK) void k_coal_sum(CoalArgs a)
{
    __shared__ uint32_t s_cnt[NWAVES];
    const int64_t t0 = (int64_t)blockIdx.x * COAL_TILE;
    uint32_t cnt = 0;
    for (int k = 0; k < COAL_ITEMS; ++k) {
        const int64_t i = t0 + k * BLOCK + threadIdx.x;
        const bool act = i < a.n;
        uint32_t s = 0;
        unsigned long long q = 0;
        bool first = false;
        if (act) {
            s = a.slot_of[i];
            q = exp_fix(a.lw[i] - max_unkey(a.gm[2 * (int64_t)s]), a.K);   // (w = m = -Inf: NaN -> 0)
            first = a.claim[s] == (uint32_t)i;
        }
        coal_add(act && q != 0, s, q, a.gm);
        cnt += (uint32_t)__popcll(__ballot(first));
    }
    if (lane_id() == 0) s_cnt[wave_id()] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int w = 0; w < NWAVES; ++w) t += s_cnt[w];
        a.tile_cnt[blockIdx.x] = t;
    }
}
// pass 3 (one workgroup): exclusive scan of the tile counts; misc[1] = number of groups
static __global__ __launch_bounds__(BLOCK) void k_coal_scan(CoalArgs a)
{
    __shared__ uint32_t s_part[BLOCK];
    const int64_t per = (a.ntiles + BLOCK - 1) / BLOCK, b0 = threadIdx.x * per;
    const int64_t b1 = b0 + per < a.ntiles ? b0 + per : a.ntiles;
    uint32_t sum = 0;
    for (int64_t b = b0; b < b1; ++b) sum += a.tile_cnt[b];
    s_part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t run = 0;
        for (int t = 0; t < BLOCK; ++t) { const uint32_t v = s_part[t]; s_part[t] = run; run += v; }
        a.misc[1] = run;
    }
    __syncthreads();
    uint32_t run = s_part[threadIdx.x];
    for (int64_t b = b0; b < b1; ++b) { const uint32_t v = a.tile_cnt[b]; a.tile_off[b] = run; run += v; }
}
// pass 4: every first member writes its group in ascending order of first occurrence: row, parent, lse_g + log(n_new / n_old)
template <int W>
__global__ __launch_bounds__(BLOCK) void k_coal_emit(CoalArgs a, double log_ratio, double* __restrict__ rows_out, double* __restrict__ lw_out,
                                                     int32_t* __restrict__ anc_out)
{
    __shared__ uint32_t s_cnt[NWAVES];
    const int64_t t0 = (int64_t)blockIdx.x * COAL_TILE;
    uint32_t run = a.tile_off[blockIdx.x];
    for (int k = 0; k < COAL_ITEMS; ++k) {
        const int64_t i = t0 + k * BLOCK + threadIdx.x;
        const bool act = i < a.n;
        uint32_t s = 0;
        bool first = false;
        if (act) { s = a.slot_of[i]; first = a.claim[s] == (uint32_t)i; }
        const unsigned long long bm = __ballot(first);
        if (lane_id() == 0) s_cnt[wave_id()] = (uint32_t)__popcll(bm);
        __syncthreads();
        uint32_t below = 0, total = 0;
        for (int w = 0; w < NWAVES; ++w) { const uint32_t v = s_cnt[w]; below += w < wave_id() ? v : 0u; total += v; }
        __syncthreads();
        if (first) {
            const int64_t j = (int64_t)run + below + (uint32_t)__popcll(bm & ((1ull << lane_id()) - 1ull));
            const double m = max_unkey(a.gm[2 * (int64_t)s]);
            const uint64_t S = a.gm[2 * (int64_t)s + 1];
            lw_out[j] = lse_from(m, S, a.K, m == -__builtin_huge_val() ? FLAG_ALL_NEGINF : 0) + log_ratio;
            anc_out[j] = (int32_t)i;
            const double2* src = reinterpret_cast<const double2*>(a.rows + i * W);
            double2* dst = reinterpret_cast<double2*>(rows_out + j * W);
#pragma unroll
            for (int c = 0; c < W / 2; ++c) dst[c] = src[c];
        }
        run += total;
    }
}

// ----------------------------------------------------------------------------- pf_introduce! (resize.jl:351-421)
// the seed of the new particles' streams: a fixed 64-bit mix of the filter's seed and the epoch of the call (gpf.h gpf_introduce)
GPF_HD uint64_t intro_seed(uint64_t seed, uint32_t epoch)
{
    uint64_t z = seed ^ ((uint64_t)epoch * 0x9e3779b97f4a7c15ull + 0xd1b54a32d192ed03ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
// the existing particles: lw += log_ml_est where it is non-zero (resize.jl:366-369), parents kept (the caller copies rows and anc)
static __global__ void k_intro_old(const double* __restrict__ lw_in, const Scalars* sc, int64_t n_old, double* __restrict__ lw_out)
{
    const double l = sc->lml_est;
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n_old; i += (int64_t)gridDim.x * BLOCK)
        lw_out[i] = l != 0.0 ? lw_in[i] + l : lw_in[i];
}
// one lane per new particle j: o_init (or the proposal) at step 1, then T - 1 steps of o_step (the proposal at the last one if PROP), the
// state in registers; RNG counter n_old + j, epochs 0 .. T-1 of the derived seed; obs = [T][MAX_OBS] (uniform loads).  parent 0 (anc -1).
template <int M, int W, bool KEEP, bool PROP>
__global__ __launch_bounds__(BLOCK) void k_introduce(ModelArgs a, uint64_t seed, const double* __restrict__ obs, int T, int64_t n_old, int64_t n,
                                                     double* __restrict__ rows_out, double* __restrict__ lw_out, int32_t* __restrict__ anc_out)
{
    using Mo = Model<M>;
    constexpr int D = Mo::D;
    for (int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x; j < n; j += (int64_t)gridDim.x * BLOCK) {
        const uint32_t gid = (uint32_t)(n_old + j);
        double x[MAX_DIM], xp[MAX_DIM];
        for (int k = 0; k < MAX_DIM; ++k) { x[k] = 0.0; xp[k] = 0.0; }
        double ll;
        if constexpr (PROP) {
            if (T == 1) ll = Mo::propose(a.P, true, nullptr, obs, seed, gid, 0, 0u, TAG_INIT, x);
            else { Mo::sample(a.P, true, nullptr, obs, seed, gid, 0, 0u, TAG_INIT, x); ll = Mo::loglik(a.P, x, obs); }
        } else {
            Mo::sample(a.P, true, nullptr, obs, seed, gid, 0, 0u, TAG_INIT, x);
            ll = Mo::loglik(a.P, x, obs);
        }
        for (int e = 1; e < T; ++e) {
            const double* ob = obs + (int64_t)e * MAX_OBS;
#pragma unroll
            for (int k = 0; k < D; ++k) xp[k] = x[k];
            double l;
            if constexpr (PROP) {
                if (e == T - 1) l = Mo::propose(a.P, false, xp, ob, seed, gid, 0, (uint32_t)e, TAG_UPDATE, x);
                else { Mo::sample(a.P, false, xp, ob, seed, gid, 0, (uint32_t)e, TAG_UPDATE, x); l = Mo::loglik(a.P, x, ob); }
            } else {
                Mo::sample(a.P, false, xp, ob, seed, gid, 0, (uint32_t)e, TAG_UPDATE, x);
                l = Mo::loglik(a.P, x, ob);
            }
            ll = ll + l;
        }
        double o[W];
#pragma unroll
        for (int k = 0; k < W; ++k) o[k] = 0.0;
#pragma unroll
        for (int k = 0; k < D; ++k) o[k] = x[k];
        if constexpr (KEEP) {
#pragma unroll
            for (int k = 0; k < D; ++k) o[D + k] = xp[k];
        }
        double2* dst = reinterpret_cast<double2*>(rows_out + (n_old + j) * W);
#pragma unroll
        for (int c = 0; c < W / 2; ++c) dst[c] = make_double2(o[2 * c], o[2 * c + 1]);
        lw_out[n_old + j] = ll;
        anc_out[n_old + j] = -1;
    }
}

} // namespace gpf
