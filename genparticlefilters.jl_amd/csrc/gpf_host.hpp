// gpf_host.hpp -- host-side internals shared by the translation units of libgpf_hip.so (libgpf_core / _resample / _aux / _blocks / _store / _shard ... .hip):
// the filter handle, the launch / error macros and the declarations of the helpers one unit defines and another calls.  Nothing here is
// part of the C ABI (include/gpf.h); everything lives in namespace gpfh and is built with hidden visibility.
#pragma once
#include "../../include/gpf.h"
#include "gpf_kernels.hpp"

#include <hip/hip_ext.h>
#include <rccl/rccl.h>        // types and enums only: librccl is loaded with dlopen (gpf_comm_create), nothing links against it
#include <dlfcn.h>
#include <unistd.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

using namespace gpf;

namespace gpfh {

// polite busy-wait on a pinned-memory ticket (x86 PAUSE; a plain compiler barrier elsewhere)
static inline void cpu_relax()
{
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#else
    __asm__ __volatile__("" ::: "memory");
#endif
}
inline thread_local std::string g_err;   // errors before a handle exists

// Kernel timing (gpf_kernel_timing): inside timed() the launch carries a start/stop event pair that the runtime
// stamps at the kernel's own begin and end (hipExtLaunchKernel), so the elapsed time is the dispatch's duration, the
// same quantity rocprofv3 --kernel-trace reports -- not launch gap + kernel as with events recorded around the launch.
inline thread_local hipEvent_t g_ev_start = nullptr, g_ev_stop = nullptr;
#define GPF_LAUNCH(kernel, grid, block, lds, stream, ...) \
    hipExtLaunchKernelGGL(kernel, grid, block, lds, stream, g_ev_start, g_ev_stop, 0, __VA_ARGS__)

struct Timer {
    bool on = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;
};
// gpf_phase_timing: events on the handle's stream at the phase boundaries of a sharded resample and of the propagate that commits it.  A mark names the
// phase that ENDS there (-1: a sequence begins); the time of a phase = from the mark in front of it, idle gaps included (GPU timeline, not kernel time).
struct PhaseTimer {
    bool on = false;
    std::vector<std::pair<int, hipEvent_t>> marks;
    double host_wait_us = 0.0;          // wall clock the host spent blocked on the exchange's split sizes
    int64_t resamples = 0;
};
// What the handle remembers about the CURRENT raw log-weights.  Three independent facts -- the maximum in the slots, a scan with its
// CDF, a reduction without one -- and the details that mean something only under their fact.  Nothing outside this struct assigns a member: the call
// sites go through the transitions below (and weights_written(), which adds the mutation counter), the producers through the three setters.
struct WeightSummary {
    bool max_valid = false;        // mslots[mcur] hold the maximum + flags of the log-weights (left by the kernel that wrote them, or by k_max_partial); always meaningful
    bool raw_valid = false;        // sc->raw = {m, flags, S} and cdf[0] with its levels / table[0] are the plain scan of the log-weights at the filter's K; always meaningful
    bool raw_has_q = false;        // only under raw_valid: that scan also accumulated sum q^2 (blockQ)
    bool raw_q_folded = false;     // only under raw_valid && raw_has_q: sc->raw.Ql is folded from blockQ (by the publishing scan or by fetch_scalars)
    bool raw_sum_valid = false;    // sum_cache = {flags, S, Ql} of the log-weights from a reduction WITHOUT a CDF (the ESS / log-ML getters, gpf_step_ess); always meaningful
    bool sum_on_host = false;      // only under raw_sum_valid: k_sum_host made it -- sum_cache holds m too and sc->raw on the device was NOT updated (else k_sum_reduce: m is in sc->raw)
    WSum sum_cache{};              // only under raw_sum_valid
    // -- transitions
    void forget() { *this = WeightSummary{}; }                    // nothing is known about the weights any more (whoever changed them answers for the mutation counter)
    void drop_sums() { const bool m = max_valid; forget(); max_valid = m; }   // sc->raw / cdf[0] were overwritten or rescaled (priorities, a sorted order, a global maximum, another K): the weights and their maximum stand
    // -- producers
    void max_produced(bool of_raw_weights) { max_valid = of_raw_weights; }   // k_max_partial filled the slots (of a priority view: they no longer describe the raw weights)
    void scanned(bool with_q, bool q_folded) { raw_valid = true; raw_has_q = with_q; raw_q_folded = q_folded; }   // ensure_raw's scan into sc->raw
    void q_folded() { raw_q_folded = true; }                      // the publish kernel folded blockQ into sc->raw.Ql
    void reduced(const WSum& w, bool on_host) { sum_cache = w; sum_on_host = on_host; raw_sum_valid = true; }   // k_sum_reduce / k_sum_host
};

// ------------------------------------------------------------------ owned memory
// `count` elements of T on the device (Dev<T>) or in pinned host memory (Pinned<T>), freed by the destructor.  Every allocation a handle owns, and every
// scratch buffer of one call, is one of these -- apart from the per-particle set (Bufs below, which is swapped whole and aliased by views) and the memory
// other processes map (the shard mailboxes and windows).  Move-only; reads as its pointer, but a kernel launch takes its arguments by value and so has
// to name the pointer (.p) -- passing the owner there does not compile.
template <class T, bool PINNED>
struct Owned {
    T* p = nullptr;
    size_t count = 0;                  // elements held
    Owned() = default;
    Owned(Owned&& o) noexcept : p(o.p), count(o.count) { o.p = nullptr; o.count = 0; }
    Owned& operator=(Owned&& o) noexcept { if (this != &o) { reset(); p = o.p; count = o.count; o.p = nullptr; o.count = 0; } return *this; }
    ~Owned() { reset(); }
    void reset()
    {
        if (p) { if (PINNED) (void)hipHostFree(p); else (void)hipFree(p); }
        p = nullptr; count = 0;
    }
    gpf_status alloc(gpf_filter* h, size_t n);                        // exactly n elements into an empty owner
    gpf_status grow(gpf_filter* h, size_t n, bool* fresh = nullptr);   // at least n: nothing, or (drain the stream, free, allocate exactly n) with *fresh = true
    operator T*() const { return p; }
    T* operator->() const { return p; }
};
template <class T> using Dev = Owned<T, false>;
template <class T> using Pinned = Owned<T, true>;

// ------------------------------------------------------------------ per-N device buffers
struct Bufs {                        // everything whose size depends on the particle count: the base of the handle, and a detached set while resizing.  Plain
    int64_t n = 0, ntiles = 0;       // pointers (free_bufs frees a set): views alias their filter's rows / lw / anc, the resize family swaps whole sets
    double* rows[2] = {nullptr, nullptr};
    int cur = 0;
    double *lw = nullptr, *lws = nullptr, *lp = nullptr, *dtmp = nullptr;
    uint64_t* cdf[3] = {nullptr, nullptr, nullptr};     // padded to whole tiles
    uint64_t* t16[3] = {nullptr, nullptr, nullptr};     // coarser levels written by the scan (gpf_kernels.hpp ScanOut)
    uint64_t* t256[3] = {nullptr, nullptr, nullptr};
    uint64_t* desc[3][2] = {{nullptr, nullptr}, {nullptr, nullptr}, {nullptr, nullptr}};   // [channel][ping-pong]: agg | prefix
    int32_t *anc = nullptr, *order = nullptr, *idx_in = nullptr;
    uint64_t *keys = nullptr, *keys_out = nullptr;
    void* sort_tmp = nullptr;
};

} // namespace gpfh

struct __attribute__((visibility("hidden"))) gpf_filter : gpfh::Bufs {
    template <class T> using Dev = gpfh::Dev<T>;
    template <class T> using Pinned = gpfh::Pinned<T>;
    gpf_config cfg{};
    ModelArgs args{};
    int d = 0, W = 0, K = 0;
    double logN = 0.0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int n_cu = 256;
    int dcur[3] = {0, 0, 0};
    const uint64_t* table[3] = {nullptr, nullptr, nullptr};   // per-tile inclusive prefixes of the last scan per channel
    size_t sort_tmp_bytes = 0;
    int sort_ws_cur = 0;
    Pinned<int64_t> h_sort_flag; int64_t sort_ticket = 0;   // pinned {a run too long for k_sort_finish, ticket}
    Dev<unsigned long long> mslots[2];                    // MaxSlots (gpf_k_common.hpp): maximum + flags of the log-weights, two alternating arrays
    int mcur = 0;                                         // mslots[mcur]: written by the latest producer
    Dev<uint64_t> blockQ;
    Dev<double> partial, dscal;
    Dev<unsigned long long> acc_part;         // [MAX_PARTIALS] accepted moves per workgroup of the last move-accept kernel
    Dev<double> tree_buf;                     // partials of the weighted tree sums (statistics)
    Dev<Scalars> sc;
    Pinned<Scalars> h_sc;          // pinned mirror
    Pinned<long long> h_sc_ticket; long long sc_ticket = 0;   // k_publish_scalars -> host polling (fetch_scalars)
    uint32_t epoch = 0;
    bool initialized = false, has_prev = false, residual_scanned = false;
    gpfh::WeightSummary summary;   // the cached summaries of the current log-weights
    Dev<uint64_t> sum_part;        // [6][workgroups] tagged partials of k_sum_reduce
    Pinned<int64_t> h_spart;       // pinned: [n_cu][8] tagged partials of k_sum_host, folded by the host
    Dev<uint64_t> gate_part; int gate_cur = 0; Pinned<int64_t> h_gate;   // gpf_step_ess: two sets of k_sum_host<GATE>'s accumulator lines (gate_verdict), pinned {ticket << 1 | verdict} of the launch that read them
    bool pending_gather = false;   // a resample left (rows[cur], anc) un-gathered; log-weights are 0
    bool pending_fill = false;     // ... or, after gpf_resample_local, the constant sc->lw_fill
    // "lazy search" (gpf_k_fused.hpp): pf_resample!(:multinomial) enqueued only the weight scan; the ancestors (h->anc) and the log-ML
    // update are still to come -- from k_step_search when a plain pf_update! follows, else from finish_search().  Implies pending_gather.
    bool pending_search = false;
    SearchArgs pend_sa{};
    // "lazy move" (gpf_k_step.hpp k_move_step): pf_rejuvenate! enqueued nothing; the move runs inside the plain pf_update! that follows
    // (gather -> move -> propagate -> one row store), or on its own (finish_move) as soon as anything else looks at the state.  The move's
    // epoch is consumed at the call (pm_epoch = the epoch the stand-alone k_move would have used).
    bool pending_move = false; int pm_method = 0, pm_iters = 0; uint32_t pm_epoch = 0; ModelArgs pm_args{};
    bool lazy_move = true;         // GPF_LAZY_MOVE=0 in the environment: every pf_rejuvenate! launches its kernel at once
    bool lazy_search = false;      // gpf_set_lazy_search (default: GPF_LAZY_SEARCH=1 in the environment, else off)
    // the 16-bit offset levels of the weight channel (k_search_multi / k_push_multi) cost the scan ~1.4 us: only written when a
    // multinomial search will read them (ScanRequest::offsets)
    bool ch0_offsets = false;      // what the last scan of channel 0 wrote
    bool offsets_hint = true;      // was the last resample multinomial?  (scans that run ahead of a resample: the ESS getter)
    bool pending_packed = false;   // sharded: the resampled population is still the received exchange buffer (gpf_shard_commit)
    const double* pend_packed = nullptr; const double* pend_mf = nullptr; const int64_t* pend_tot = nullptr; int pend_G = 0;
    bool pend_mailbox = false;     // pend_mf / pend_tot sit in the shard mailbox
    // own-direct commit (k_search_own): the packed buffer holds pend_m < n entries (the slots other shards serve), the shard's own hits
    // sit in h->anc as global ancestor ids (-1 elsewhere) and are gathered through it
    bool pend_own = false; int64_t pend_m = 0; bool pend_own_range = false;   // (own hits named by ShardPlan::own_range: stratified)
    // trajectory store (gpf_history_enable): per recorded step the d latent columns in the step's final particle
    // order, and the composed ancestor map of the resamples that happened during that step (nullptr = identity)
    bool hist_on = false;
    bool hist_blocks = false;            // gpf_history_enable_blocks: the block-wise calls feed the store too (the plain store refuses them)
    int hist_cap = 0;
    std::vector<Dev<double>> hist_x;     // [step] n*d doubles (empty until snapshotted)
    std::vector<Dev<int32_t>> hist_map;  // [step] n int32 or empty
    int hist_step = -1;                  // index of the current step (0 = after gpf_initialize)
    Dev<const int32_t*> hist_dev_maps;
    Dev<const double*> hist_dev_x;         // device table of the snapshots hist_x[s], hist_cap entries (gpf_block_sample_trajectories walks all steps in one launch)
    // gpf_history_enable_blocks_weights: what a backward pass needs of every step, taken wherever hist_snapshot takes hist_x (none of it exists otherwise)
    bool hist_weights = false;
    // (both live behind the step's columns in the allocation of hist_x[step]: nothing of their own to free)
    std::vector<double*> hist_lw;        // [step] the n log-weights in the step's final order (nullptr until snapshotted)
    std::vector<double*> hist_obs;       // [step] the [n_blocks][MAX_OBS] observation rows the step was entered with, in the block order of the snapshot
    std::vector<int64_t> hist_bsize;     // [step] the block size of the block-wise call that entered the step; 0: a whole-filter call (no per-block rows)
    Dev<const double*> hist_dev_lw, hist_dev_obs;   // device tables of hist_lw / hist_obs beside hist_dev_x, hist_cap entries each
    // forward-only smoothing per block (gpf_forward_enable_blocks): ONE generation of records -- the previous step's latent columns,
    // log-weights and statistics in that step's final order -- and the composed ancestor map of the current step; 8 (2 F + d + 1) n bytes and two maps,
    // however long the series.  Everything is allocated by the initialising call and overwritten at every close (fwd_begin_step)
    bool fwd_on = false;
    int64_t fwd_bsize = 0;               // the (clamped) block size of the initialising call: the mode's; 0 until then
    int32_t fwd_steps = 0;               // the current step, 1-based; 0: nothing initialised
    Dev<double> fwd_x, fwd_lw;           // [n][d], [n] of the step closed last: fwd_lw.count = the particles the records hold
    Dev<double> fwd_T[2]; int fwd_cur = 0;   // [n][F]: fwd_T[fwd_cur] belongs to the record, the other half is the close's output and the query's scratch
    Dev<int32_t> fwd_map[2]; int fwd_map_cur = 0; bool fwd_map_set = false;   // g_s of the current step in fwd_map[fwd_map_cur] once a resample happened in it
    // sub-state view (src/view.jl:16-48): this handle aliases particles [view_start, view_start + n) of `parent`
    gpf_filter* parent = nullptr;
    std::vector<gpf_filter*> views;      // the live view handles of THIS filter: gpf_destroy orphans them (a view used after its filter is gone fails loudly)
    bool orphaned = false;               // view: its filter was destroyed -- parent dangles and is never followed, the stream is gone with it
    int64_t view_start = 0;
    int64_t view_step = 1;               // > 1: strided view (state[start:step:stop]); works on the compact copies below
    Dev<double> vrows[2], vlw; Dev<int32_t> vanc;
    Dev<int32_t> vidx, vgid;             // view over an index vector (view_step == 0): the particles' indices in the parent, and idx - idx[0] (ModelArgs::gid_map)
    uint64_t generation = 0;             // bumped when the per-particle buffers are reallocated (views check it)
    uint64_t parent_generation = 0;
    uint64_t mutations = 0;              // bumped by every change of the rows / log-weights of this filter (through any handle)
    uint64_t seen_mutations = 0;         // view: the parent's counter when this view's cached summaries were valid
    // multi-GPU: the library's own RCCL communicator and the device scratch of gpf_shard_resample
    ncclComm_t comm = nullptr;
    int comm_rank = 0, comm_world = 1;
    double *sh_mf = nullptr, *sh_mf_all = nullptr; int64_t *sh_tot = nullptr, *sh_tot_all = nullptr, *sh_cr = nullptr, *sh_cr_all = nullptr;
    Dev<double> sh_send, sh_recv;        // the exchange buffers: released with the communicator (gpf_comm_destroy)
    // shard mailboxes (gpf_k_common.hpp): the three small summaries of a sharded resample travel as peer stores from the
    // producing kernel into every rank's mailbox instead of RCCL all-gathers
    uint64_t* mbox = nullptr;            // this rank's mailbox (device memory, exported through hipIpc)
    uint64_t** mb_peers = nullptr;       // device array [world]: every rank's mailbox as mapped in this process
    std::vector<void*> mb_opened;        // peers' mailboxes opened with hipIpcOpenMemHandle (closed by gpf_comm_destroy)
    bool mb_active = false;
    bool mb_fuse_default = false;        // every rank of the communicator has a device of its own: the (max, flags) round rides in its consumer's launch (mailbox_fuse_mf)
    // the GLOBAL weight summary of the latest one-launch reduction (k_sum_shard: the sharded ESS getter / gpf_shard_step_ess), as the host read it, and what
    // it describes: a gpf_shard_resample that finds it still valid (same weights, no newer mailbox round) does not repeat the (max, flags) round, and a
    // residual one runs no weight scan at all (shard_resample_impl)
    bool gsum_ok = false; uint64_t gsum_mut = 0, gsum_mf_seq = 0, gsum_tot_seq = 0; WSum gsum{};
    bool comm_poisoned = false;          // a sharded call failed on THIS rank after its mailbox rounds / collectives had begun: the peers are out of step with it
    // the slot-addressed receive window (gpf_k_common.hpp RingOut / RingIn): one entry of W + 2 words per local slot and parity, mapped by every peer
    uint64_t* ring = nullptr;            // this rank's window (device memory, exported through hipIpc)
    uint64_t** ring_peers = nullptr;     // device array [world]: every rank's window as mapped in this process
    std::vector<void*> ring_opened;
    bool ring_active = false;
    int64_t ring_parity_words = 0;       // words of one parity: (slots of the largest shard) x (W + 2)
    uint64_t ring_seq = 0;               // window exchanges so far: the same on every rank (SPMD call order)
    int exchange_mode = 0;               // gpf_comm_set_exchange: GPF_SHARD_EXCHANGE_RCCL | _P2P (the resamplers with ascending targets)
    bool pend_ring = false; uint64_t pend_ring_seq = 0;   // the pending commit's entries sit in the window (exchange pend_ring_seq)
    int64_t* tr_dev = nullptr;           // device {entries sent, received} of the window exchanges (the host never learns their counts: gpf_comm_traffic reads these)
    uint64_t sh_round = 0;               // summary rounds so far: the local / gathered arrays are rings of SH_RING rounds
    const double* cur_mf_all = nullptr; const int64_t* cur_tot_all = nullptr; const int64_t* cur_cr_all = nullptr;   // the gathered summaries of the current round
    uint64_t mb_seq[MB_KINDS] = {0, 0, 0, 0};   // rounds so far per kind: the same on every rank (SPMD call order)
    uint64_t mb_cur[MB_KINDS] = {0, 0, 0, 0};   // the round whose entries the current gathered pointers name
    Pinned<int32_t> h_timeout;           // pinned: set by a scan whose bounded inter-workgroup wait gave up (checked on the host)
    int scan_blocks_per_cu = 2;          // resident scan workgroups per CU the launch may rely on (occupancy query)
    int wscan_blocks_per_cu = 2;         // ... of the weight scans k_scan<InFixQ, *> alone (fewer registers than the residual scan)
    Dev<int64_t> shard_counts;           // [2 * MAX_SHARDS] exchange counters of the current resample (device) + pinned mirror
    Pinned<int64_t> h_shard_counts;
    // block-wise resampling (gpf_resample_blocks): {flags, count} words, the per-block mask, per-block statistics
    Pinned<int64_t> h_qpub; int64_t q_ticket = 0;   // the ESS getter's scan publishes {flags, S, limbs of sum q^2} itself (ScanExtras::q_host)
    Dev<int32_t> blk_words, blk_mask; Dev<double> blk_stats; int64_t blk_last = 0;   // (mask and statistics grow together: [n_blocks], [n_blocks][2])
    Dev<double> blk_est;                                        // per-block estimates (gpf_block_moments / gpf_block_proportion)
    // blocks of more than BLK_MAX particles: gpf_resample_blocks / gpf_block_stats run the loop over sub-states themselves, through view
    // handles kept on the filter (one per block; rebuilt when the block size or the particle buffers change)
    std::vector<gpf_filter*> blk_views; int64_t blk_views_size = 0; uint64_t blk_views_gen = 0;
    Dev<double> blk_obs;                                                               // per-block observations [n_blocks][MAX_OBS] on the device
    static constexpr int BLK_STAGE = 4;                                                // pinned staging buffers, used in turn (no stream sync per step)
    Pinned<double> h_blk_obs[BLK_STAGE];
    int64_t blk_stage_next = 0;                                                        // staging copies issued so far (ticket of the next one - 1)
    Pinned<int64_t> h_blk_done; Dev<unsigned int> blk_stage_counter;                   // pinned: ticket of the last finished staging copy; device: its workgroup counter
    int64_t blk_obs_size = 0;                                                          // > 0: the latest observations are per block, blocks of this size
    // conditional SMC (gpf_initialize_blocks_ref / gpf_update_blocks_ref): the reference rows of the CURRENT call, [n_blocks][MAX_DIM] on the device
    // (ModelArgs::blk_ref for the one launch).  They are staged behind the observations in the same pinned buffer (h_blk_obs holds MAX_OBS + MAX_DIM
    // words per block) and copied by the same launch; nothing of them is kept between calls
    Dev<double> blk_ref;
    // ancestor sampling (gpf_resample_blocks_ancestor / gpf_block_ancestor_log_weights): the data vectors and reference values of the step being ENTERED,
    // [n_blocks][MAX_OBS] then [n_blocks][MAX_DIM] on the device -- scratch of the one call, apart from blk_obs (a rejuvenation before the update still
    // sees the previous step's observation).  h_anc_in: the pinned buffer the copy kernel reads; anc_ev: recorded behind that kernel, waited for before
    // the buffer is filled again
    Dev<double> anc_in; Pinned<double> h_anc_in; hipEvent_t anc_ev = nullptr; bool anc_ev_pending = false;
    // gpf_set_block_params: every block's own model parameters, [n_blocks][MAX_PARAMS] on the device (ModelArgs::blk_params), uploaded once;
    // bp_size > 0: the rows are in force for blocks of this (clamped) size -- the block-wise steps run their BP kernels, everything that would
    // read cfg.params is refused (bp_refused)
    Dev<double> blk_params; int64_t bp_size = 0;
    // gpf_run_blocks: the call's device input [MAX_PARAMS parameters | n_steps x (n_blocks | 1) x MAX_OBS observations] with the pinned buffer it is
    // packed into, and its outputs [ess | lml] x [n_steps][n_blocks], [n_steps][n_blocks] resample words.  Scratch of one call (it ends with a
    // synchronisation), kept for the next
    Dev<double> run_in, run_stats; Pinned<double> h_run_in; Dev<int32_t> run_words;
    // gpf_resample_across_blocks: the planner filter of n_blocks particles whose log-weights are the blocks' log-ML estimates (its ancestors name the
    // source block of every block; it runs on this filter's stream), the second buffers the per-block rows are gathered into (swapped with
    // blk_params / blk_obs), and the 1-based block ancestors of the last call that fired with the buffers they refer to (gpf_block_ancestors)
    gpf_filter* xb_planner = nullptr;
    Dev<double> blk_params_alt, blk_obs_alt;
    std::vector<int64_t> xb_anc; uint64_t xb_anc_gen = 0; int64_t xb_anc_n = 0;
    // the pull plan (gpf_comm_set_plan): request lists [G][n], their counters, the dense / gathered request matrix and its pinned mirror
    int shard_plan_kind = 0;
    Dev<ulonglong2> pull_req;
    Dev<int64_t> pull_counts, pull_pc, pull_pc_all; Pinned<int64_t> h_pull_pc_all;
    Pinned<int64_t> h_flags;             // pinned {validity flags, ticket} published by the weight scan of a checked resample
    int64_t flag_ticket = 0;
    int64_t push_ticket = 0;             // bumped by every gpf_shard_push launch; k_push publishes it with the counts
    bool counts_published = false;
    // GPF_RESAMPLE_MULTINOMIAL_SORTED: gamma totals of the tiles of SP_TILE slots (k_sorted_gammas) and, for many tiles, their starting points (k_sorted_tiles)
    Dev<uint64_t> sp_g, sp_vlo;          // (grown together)
    SortedGammaJob sp_job{};             // the latest job that draws them (sorted_job_prepare): a weight scan of the same call carries it (ScanRequest::sp), else k_sorted_gammas
    Dev<ulonglong2> push_stage;          // push exchange: staged hits, one 16-byte entry per global output slot at most
    // sharded stratified resampling with sort_particles = true (gpf_shard_resample_sorted; gpf_k_shard.hpp AncPlan): the planner filter of n_global particles
    // every rank sorts / scans / searches the gathered log-weights with, the all-gather staging of unequal shards, the pack cursors
    gpf_filter* planner = nullptr;
    Dev<double> sorted_src, sorted_gath;
    Dev<unsigned long long> anc_cursors;
    Dev<ShardPlan> shard_plan;           // sharded stratified / sorted multinomial resampling: the slot range this shard serves (k_strat_plan, k_sorted_plan)
    Dev<int64_t> splan_F; Dev<unsigned int> splan_arrive;   // k_sorted_plan: boundary scratch [MAX_SHARDS + 1], arrival counter (zero between launches)
    bool push_counted = false;
    // exchange volume of the sharded resamples so far (gpf_comm_traffic): calls, entries sent to / received from OTHER ranks, bytes of one entry of the latest call
    int64_t tr_calls = 0, tr_sent = 0, tr_recv = 0, tr_entry_bytes = 0;
    int last_flags = 0;                  // safe_softmax flags (FLAG_*) of the latest resample that read them on the host (resample_impl)
    hipEvent_t chain_ev = nullptr;       // ChainGate: recorded behind this filter's chained kernels while other filters live on the device
    bool chain_counted = false;
    gpfh::Timer timers[GPF_K_COUNT];
    gpfh::PhaseTimer phases;
    std::string err;
};

namespace gpfh {

#define HIP_TRY(h, expr)                                                                        \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess) {                                                                 \
            (h)->err = std::string(#expr) + ": " + hipGetErrorString(e_);                       \
            return GPF_ERR_HIP;                                                                 \
        }                                                                                       \
    } while (0)

inline gpf_status fail(gpf_handle h, gpf_status s, const std::string& msg)
{
    if (h) h->err = msg; else g_err = msg;
    return s;
}

// Poll pinned memory that a kernel on h->stream publishes into, until ready() holds.  A failed kernel never publishes: any stream status other than
// "not ready" is terminal (ready() once more, then report), so a faulting kernel cannot hang the host -- or, in a multi-rank job, its peers in the
// next collective.  The failure text: [what: ] + `drained` when the stream is idle and nothing came, else the stream's own error.
// (see Owned above) a failed allocation leaves the owner empty and the HIP error in h->err; the next call tries again
template <class T, bool PINNED>
gpf_status Owned<T, PINNED>::alloc(gpf_filter* h, size_t n)
{
    if (PINNED) HIP_TRY(h, hipHostMalloc(&p, n * sizeof(T))); else HIP_TRY(h, hipMalloc(&p, n * sizeof(T)));
    count = n;
    return GPF_OK;
}
// grow-only: kernels enqueued earlier may still read the old buffer, so the stream drains before it is freed.  No geometric growth
template <class T, bool PINNED>
gpf_status Owned<T, PINNED>::grow(gpf_filter* h, size_t n, bool* fresh)
{
    if (count >= n) return GPF_OK;
    if (p) { HIP_TRY(h, hipStreamSynchronize(h->stream)); reset(); }
    if (fresh) *fresh = true;
    return alloc(h, n);
}

template <class Ready>
gpf_status poll_published(gpf_filter* h, Ready&& ready, const char* what, const char* drained)
{
    uint64_t spins = 0;
    while (!ready()) {
        cpu_relax();
        if ((++spins & 0x3fff) != 0) continue;
        const hipError_t q = hipStreamQuery(h->stream);
        if (q == hipErrorNotReady) continue;
        if (ready()) break;
        return fail(h, GPF_ERR_HIP, (what ? std::string(what) + ": " : std::string()) + (q == hipSuccess ? drained : hipGetErrorString(q)));
    }
    return GPF_OK;
}
inline gpf_status wait_ticket(gpf_filter* h, volatile int64_t* tk, int64_t want, const char* what)
{ return poll_published(h, [&] { return __atomic_load_n(tk, __ATOMIC_ACQUIRE) == want; }, what, "the stream drained without the ticket being published"); }
// a lazily allocated block of n pinned words a kernel publishes into (flags, tickets, summaries), zeroed
inline gpf_status pinned_words(gpf_filter* h, Pinned<int64_t>& words, int n)
{
    if (!words) { if (gpf_status s = words.alloc(h, (size_t)n)) return s; std::fill(words.p, words.p + n, (int64_t)0); }
    return GPF_OK;
}

// gpf_set_block_params: while the rows are set on a filter, a call on it or on a view of it that would use the filter's one parameter vector fails
inline gpf_status bp_refused(gpf_filter* h, const char* who)
{
    const gpf_filter* root = (h->parent && !h->orphaned) ? h->parent : h;
    if (root->bp_size > 0)
        return fail(h, GPF_ERR_STATE, std::string(who) + ": per-block model parameters are set (gpf_set_block_params): use the block-wise calls, or clear them first");
    return GPF_OK;
}

// gpf_forward_enable_blocks: while the mode is on, the calls that would scatter the blocks' lineages or replace the population are refused
inline gpf_status fwd_refused(gpf_filter* h, const char* who)
{
    if (h->fwd_on)
        return fail(h, GPF_ERR_STATE, std::string(who) + ": forward smoothing per block is on (gpf_forward_enable_blocks): the statistics follow the block-wise calls only");
    return GPF_OK;
}

constexpr int row_width(int D, bool keep) { return ((keep ? 2 * D : D) + 1) & ~1; }
// one buffer per scan channel: the per-256 level (8 u64 per tile), the 4-byte key level (64 u32 per tile), the 16-bit
// in-group offsets (2048 u16 per tile) and their coarse rows (<= 512 u16 per tile) -- gpf_kernels.hpp ScanOut
// ... and, beyond 2.5 M particles, the compact copy of every 4th / 8th / 16th key (<= 16 u32 per tile)
inline size_t t256_bytes(int64_t ntiles) { return (size_t)ntiles * ((TILE / 256) * sizeof(uint64_t) + (TILE / 32) * sizeof(uint32_t) + TILE * sizeof(uint16_t) + (TILE / 4) * sizeof(uint16_t) + 16 * sizeof(uint32_t)); }
inline uint32_t* k32_of(uint64_t* t256, int64_t ntiles) { return reinterpret_cast<uint32_t*>(t256 + ntiles * (TILE / 256)); }
inline uint16_t* off16_of(uint64_t* t256, int64_t ntiles) { return reinterpret_cast<uint16_t*>(k32_of(t256, ntiles) + ntiles * (TILE / 32)); }
inline uint16_t* coarse_of(uint64_t* t256, int64_t ntiles) { return off16_of(t256, ntiles) + ntiles * TILE; }
inline uint32_t* k32s_of(uint64_t* t256, int64_t ntiles) { return reinterpret_cast<uint32_t*>(coarse_of(t256, ntiles) + ntiles * (TILE / 4)); }
// channel 0 (the weights) carries the offset levels when k_search_multi can take the filter (multi_logg >= 0)
inline ScanOut scan_out(uint64_t* cdf, uint64_t* t16, uint64_t* t256, int64_t ntiles, bool with_offsets)
{
    int logg = with_offsets ? multi_logg(ntiles) : -1;
    const int sample = with_offsets && logg < 0 ? multi_sample(ntiles) : 0;       // beyond 2.5 M particles: 32-cell levels + sampled keys
    if (sample > 0) logg = 0;
    return ScanOut{cdf, t16, t256, k32_of(t256, ntiles), logg >= 0 ? off16_of(t256, ntiles) : nullptr, logg >= 0 ? coarse_of(t256, ntiles) : nullptr, logg,
                   sample > 0 ? k32s_of(t256, ntiles) : nullptr, sample};
}

inline int grid_for(const gpf_filter* h, int64_t work_items, int blocks_per_cu)
{
    const int64_t need = (work_items + BLOCK - 1) / BLOCK;
    const int64_t cap = (int64_t)h->n_cu * blocks_per_cu;
    return (int)std::max<int64_t>(1, std::min(need, cap));
}

// the slots the next producer of log-weights folds its maximum into (and the array it clears for the producer after it)
inline MaxSlots next_slots(gpf_filter* h) { h->mcur ^= 1; return MaxSlots{h->mslots[h->mcur], h->mslots[1 - h->mcur]}; }

template <class F>
gpf_status timed(gpf_filter* h, int id, F&& launch)
{
    Timer& t = h->timers[id];
    if (!t.on) { launch(); return GPF_OK; }
    hipEvent_t a, b;
    HIP_TRY(h, hipEventCreate(&a));
    HIP_TRY(h, hipEventCreate(&b));
    g_ev_start = a; g_ev_stop = b;
    launch();                       // exactly one GPF_LAUNCH
    g_ev_start = g_ev_stop = nullptr;
    t.ev.emplace_back(a, b);
    return GPF_OK;
}

// ------------------------------------------------------------------ chained kernels of SEVERAL filters on one device
// The scans (k_scan, k_scan_residual2) and the sort's partition passes (k_sort_pass) chain their workgroups: a workgroup waits for the prefix of the tiles
// below its own.  With ONE such kernel on the device that is safe -- its grid is sized to be resident at once (resample_device_setup), and a workgroup
// only ever waits for workgroups dispatched before it.  TWO of them in flight on different streams (independent filters stepped from one process:
// tools/replicas.py, R = 4 filters of 2 x 10^6 particles) can each hold the slots the other's not-yet-dispatched workgroups need: every resident
// workgroup waits, nothing retires -- the bounded spins give up after seconds and the run fails loudly ("bounded inter-workgroup wait timed out").
// So: while a process holds MORE THAN ONE filter on a device, its chained kernels run one after the other -- each such launch waits for the event
// behind the previous one (of whichever stream) and records its own.  Everything else (propagate, search, gather, reductions) still overlaps across
// the streams, and a process with one filter per device -- the headline, every sharded rank -- never touches the gate.
struct ChainGate {
    std::mutex mu;
    int live = 0;                        // filters (not views) alive on the device
    hipEvent_t last = nullptr;           // behind the latest chained launch ...
    hipStream_t last_stream = nullptr;   // ... which went to this stream
};
inline ChainGate g_chain[16];
struct ChainScope {                      // around the launch (or the launches, same stream) of chained kernels
    gpf_filter* h; ChainGate* g; bool on;
    explicit ChainScope(gpf_filter* f);
    ~ChainScope();
};

inline void phase_mark(gpf_filter* h, int id)
{
    if (!h->phases.on) return;
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) return;
    (void)hipEventRecord(e, h->stream);
    h->phases.marks.emplace_back(id, e);
}

inline ChainScope::ChainScope(gpf_filter* f) : h(f), g(nullptr), on(false)
{
    const int dev = h->cfg.device;
    if (dev < 0 || dev >= 16) return;
    g = &g_chain[dev];
    g->mu.lock();
    on = g->live > 1;
    if (on && g->last && g->last_stream != h->stream) (void)hipStreamWaitEvent(h->stream, g->last, 0);
}
inline ChainScope::~ChainScope()
{
    if (!g) return;
    if (on) {
        gpf_filter* owner = h->parent ? h->parent : h;            // (a view launches on its filter's stream; the event lives with the filter)
        if (!owner->chain_ev && hipEventCreateWithFlags(&owner->chain_ev, hipEventDisableTiming) != hipSuccess) owner->chain_ev = nullptr;
        if (owner->chain_ev && hipEventRecord(owner->chain_ev, h->stream) == hipSuccess) { g->last = owner->chain_ev; g->last_stream = h->stream; }
    }
    g->mu.unlock();
}

// ------------------------------------------------------------------ shard mailboxes (host side)
// begin a new round of `kind` (the producing kernel of this call pushes it); no mailbox / not the library engine (ShardCall::engine): push nowhere
inline MboxPush mb_begin(gpf_filter* h, bool engine, int kind)
{
    MboxPush p{};
    if (!(h->mb_active && engine)) return p;
    const uint64_t seq = ++h->mb_seq[kind];
    h->mb_cur[kind] = seq;
    const int slot = (int)(seq & (MB_SLOTS - 1));
    p.peers = h->mb_peers; p.payload_off = mb_payload_off(kind, slot); p.tag_off = mb_tag_off(kind, slot);
    p.tag = seq; p.G = h->comm_world; p.me = h->comm_rank; p.nwords = mb_words(kind);
    return p;
}
// what a consumer of the current round of `kind` waits for
inline MboxWait mb_wait(const gpf_filter* h, bool engine, int kind)
{
    MboxWait w{};
    if (!(h->mb_active && engine)) return w;
    const uint64_t seq = h->mb_cur[kind];
    w.tags = h->mbox + mb_tag_off(kind, (int)(seq & (MB_SLOTS - 1))); w.want = seq; w.n = h->comm_world; w.nwords = mb_words(kind); w.timeout = h->h_timeout;
    return w;
}
// the gathered array of the current round of `kind` inside the own mailbox ([G][words], dense like the all-gather's output)
inline const void* mb_gathered(const gpf_filter* h, int kind)
{
    return h->mbox + mb_payload_off(kind, (int)(h->mb_cur[kind] & (MB_SLOTS - 1)));
}

#ifndef STEP_BLOCKS_PER_CU
#define STEP_BLOCKS_PER_CU 4
#endif
inline int step_grid(const gpf_filter* h) { return std::min(grid_for(h, h->n, STEP_BLOCKS_PER_CU), MAX_PARTIALS); }
// the rejuvenation kernels: rounds 1-2 found them FASTER with fewer workgroups per CU (8 per CU 105 / 123 us, 2: 52 / 61, bearings MH / SV
// move-reweight) -- the reason was one same-address atomic per WAVE for the accept count (~10 ns each, serialised: 20-40 us).  With
// per-workgroup counts (round 3): 2 per CU 36.7 / 44.2 us, 3: 32.1 / 44.6, 4: 31.3 / 44.6, 6: 31.2 / 47.7, 8: 31.5 / 47.0.
#ifndef MOVE_BLOCKS_PER_CU
#define MOVE_BLOCKS_PER_CU 4
#endif
inline int move_grid(const gpf_filter* h) { return std::min(grid_for(h, h->n, MOVE_BLOCKS_PER_CU), MAX_PARTIALS); }

#define DISPATCH_MODEL(h, CALL)                                                                  \
    switch ((h)->cfg.model) {                                                                    \
        case MODEL_LGSSM2: { constexpr int MM = MODEL_LGSSM2; CALL; } break;                     \
        case MODEL_BEARINGS4: { constexpr int MM = MODEL_BEARINGS4; CALL; } break;               \
        case MODEL_SV1: { constexpr int MM = MODEL_SV1; CALL; } break;                           \
        case MODEL_OBJECT_MOTION: { constexpr int MM = MODEL_OBJECT_MOTION; CALL; } break;       \
        case MODEL_LINE: { constexpr int MM = MODEL_LINE; CALL; } break;                         \
    }
// the row width of the filter (2, 4 or 8 doubles) as constexpr int WW
#define DISPATCH_W(h, CALL)                                                                      \
    switch ((h)->W) {                                                                            \
        case 2: { constexpr int WW = 2; CALL; } break;                                           \
        case 4: { constexpr int WW = 4; CALL; } break;                                           \
        case 8: { constexpr int WW = 8; CALL; } break;                                           \
    }
// the latent dimension of the filter (1, 2 or 4 columns; the caller has refused any other) as constexpr int DD
#define DISPATCH_D(h, CALL)                                                                      \
    switch ((h)->d) {                                                                            \
        case 1: { constexpr int DD = 1; CALL; } break;                                           \
        case 2: { constexpr int DD = 2; CALL; } break;                                           \
        case 4: { constexpr int DD = 4; CALL; } break;                                           \
    }

// f(std::bool_constant<a>{}[, std::bool_constant<b>{}]): runtime flags as template arguments, e.g. launch_x<MM, KEEP, BP> with KEEP, BP the arguments
template <class F>
inline void bool_dispatch(bool a, F&& f)
{
    if (a) f(std::true_type{}); else f(std::false_type{});
}
template <class F>
inline void bool_dispatch(bool a, bool b, F&& f)
{
    bool_dispatch(a, [&](auto A) { bool_dispatch(b, [&](auto B) { f(A, B); }); });
}

// what the filter's model offers beyond its default sampler (gpf_models.hpp Model<M>::HAS_*)
struct ModelCaps { bool proposal, strata, strata_proposal, move_proposal; };
inline ModelCaps model_caps(const gpf_filter* h)
{
    ModelCaps c{};
    DISPATCH_MODEL(h, (c = ModelCaps{Model<MM>::HAS_PROPOSAL, Model<MM>::HAS_STRATA, Model<MM>::HAS_STRATA_PROPOSAL, Model<MM>::HAS_MOVE_PROPOSAL}));
    return c;
}
// does the native proposal id name this model's proposal: the locally optimal one (all models but line_model), the reference tests' fixed
// proposals (line_model).  Whether the model has a native proposal at all is model_caps(h).proposal.
inline bool proposal_valid(const gpf_filter* h, int32_t proposal)
{
    if (proposal == GPF_PROPOSAL_LOCALLY_OPTIMAL) return h->cfg.model != MODEL_LINE;
    if (proposal == GPF_PROPOSAL_LINE_FIXED) return h->cfg.model == MODEL_LINE;
    return false;
}

inline PrioView raw_view(const gpf_filter* h) { return PrioView{h->lw, nullptr, 0.0, 0}; }

// ------------------------------------------------------------------ per-call options (arguments, not state: the handle keeps only what outlives a call)
// What one weight-scan launch is to produce (scan_launch, summarize).  The default: the CDF with its offset levels, one k_max_partial pass in front.
struct ScanRequest {
    bool cdf = true;                     // the CDF and its coarser levels (else the sums alone)
    bool q = false;                      // also accumulate sum q^2 (only the ESS needs it)
    bool publish_flags = false;          // the validity flags go to pinned memory (h_flags, flag_ticket)
    bool max_ready = false;              // the maximum slots describe the weights already (the sorted resample needs the maximum for its sort keys) ...
    bool producer_max = false;           // ... else: the slots of the kernel that produced the raw log-weights will do while they are current (ensure_max)
    bool offsets = true;                 // the 16-bit offset levels of channel 0 (~1.4 us: only a multinomial search / push reads them)
    const int32_t* order = nullptr;      // scan in this order (after sort_desc: the sorted keys are in h->keys)
    const SortedGammaJob* sp = nullptr;  // a sorted multinomial resample's tile totals ride in this launch as extra workgroups
};
// What the caller of the sharded phases wants of them.  The default is a public phase call (gpf_shard_weight_max ... gpf_shard_commit, one by one from
// sharded.py): no mailbox, nothing resolved in place, no windows, no plan in the scan's launch, the raw weights into sc->raw with a CDF, no extra field.
// The library engine (shard_resample_impl, gpf_shard_step_ess, the sharded getters) builds one per call and passes it down.
struct ShardCall {
    bool engine = false;                 // the phases push / wait through the shard mailboxes when they are up (mb_begin / mb_wait)
    bool own = false;                    // own hits are resolved in place: ancestors into h->anc, only the other shards' slots travel
    bool own_range = false;              // ... stratified / sorted multinomial: they are one slot range (ShardPlan::own_range), written by k_search_strat's pack loop
    bool ring = false;                   // the rows go through the receive windows
    bool plan_in_scan = false;           // stratified: the plan rides in the weight scan's launch (k_scan MODE 3, ScanExtras::splan) ...
    bool plan_rode = false;              // ... and did (written by the weight scan for the push count of the same call: no k_strat_plan)
    bool gammas_pending = false;         // sorted multinomial: h->sp_job is still to be drawn -- by the next weight scan, else by the push count
    bool offsets = true;                 // ScanRequest::offsets of the weight scans
    const PrioView* view = nullptr;      // summarise this view of the weights (a prioritised resample: alpha lw, then log_ws) instead of the raw ones ...
    WSum* slot = nullptr;                // ... into this slot instead of sc->raw ...
    bool cdf = true;                     // ... with or without the CDF
    int extra = 0; PrioView extra_pv{nullptr, nullptr, 0.0, 0};   // the extra field of a prioritised entry (PushArgs::extra / pv)
};

// ------------------------------------------------------------------ weight summary = (max) + scan
// The scan's inter-workgroup protocol needs every workgroup of the launch resident at once (block b owns tiles b, b + G, ...
// and waits for lower tiles of its round): at most scan_blocks_per_cu per CU, from the occupancy query at gpf_create.
inline int scan_grid(const gpf_filter* h) { return (int)std::max<int64_t>(1, std::min<int64_t>(h->ntiles, (int64_t)h->scan_blocks_per_cu * h->n_cu)); }
// the weight scans (k_scan<InFixQ, *>): up to WSCAN_MAX workgroups per CU, so that filters of up to WSCAN_MAX x 0.52 M particles scan in ONE round
inline int wscan_grid(const gpf_filter* h) { return (int)std::max<int64_t>(1, std::min<int64_t>(h->ntiles, (int64_t)h->wscan_blocks_per_cu * h->n_cu)); }

inline void normalise_Q(const WSum& w, uint64_t& hi, uint64_t& lo)
{
    unsigned __int128 Q = (unsigned __int128)w.Ql[0] + ((unsigned __int128)w.Ql[1] << 32) +
                          ((unsigned __int128)w.Ql[2] << 64) + ((unsigned __int128)w.Ql[3] << 96);
    hi = (uint64_t)(Q >> 64);
    lo = (uint64_t)Q;
}


// ---- defined in libgpf_core.hip
Bufs take_particle_buffers(gpf_filter* h);
void free_bufs(Bufs& b);
gpf_status alloc_particle_buffers(gpf_filter* h, bool scratch_only = false);
gpf_status alloc_fixed_buffers(gpf_filter* h);
void launch_gather_ex(gpf_filter* h, const int32_t* anc, const double* in, double* out, const PrioView& pv, double* lw_out, int64_t n);
void launch_gather(gpf_filter* h, const PrioView& pv, double* lw_out);
void launch_gather_rows_lw(gpf_filter* h, const int32_t* anc, const double* rows_in, const double* lw_in, double* rows_out, double* lw_out, int64_t n);
gpf_status materialize(gpf_filter* h);
gpf_status finish_move(gpf_filter* h);
void hist_clear(gpf_filter* h);
gpf_status hist_snapshot(gpf_filter* h);
gpf_status hist_on_resample(gpf_filter* h, int64_t block_size = 0);
gpf_status hist_begin_step(gpf_filter* h, bool first);
void mutated(gpf_filter* h);
void weights_written(gpf_filter* h, bool max_in_slots);
gpf_status after_initialize(gpf_filter* h, int grid);
void after_propagate(gpf_filter* h);
gpf_status view_enter(gpf_filter* v);
gpf_status view_exit(gpf_filter* v);
gpf_status check_ready(gpf_handle h, bool keep_pending_move = false);
gpf_status set_obs(gpf_filter* h, const double* obs, int n_obs);
gpf_status copy_out(gpf_handle h, const void* dsrc, void* out, size_t bytes);
gpf_status set_strata(gpf_handle h, const double* values, int32_t n_strata, int32_t interleaved);
gpf_status speculative_step(gpf_filter* h, const GateIn& gate);
void speculative_step_done(gpf_filter* h, bool ran);
// ---- defined in libgpf_resample.hip
// one scan launch on descriptor channel `ch` (0 weights, 1 residual counts, 2 residual weights): the sharded weight scans (MODE 3: pushes
// the shard's total itself; 4: also the limbs of sum q^2) and the scans of pf_optimal_resize!
gpf_status scan_launch_shard(gpf_filter* h, int mode, const InFixQ& in, int np, WSum* slot, const ScanRequest& rq, uint64_t* total_out, const double* mf_all, const ScanExtras& ex);
gpf_status scan_launch_optimal(gpf_filter* h, int ch, const InOptimal& in, uint64_t* total_out);
gpf_status resample_device_setup(gpf_filter* h);      // occupancy of the scan kernels, LDS attributes of the searches (gpf_create)
gpf_status ensure_max(gpf_filter* h, const PrioView& pv, bool use_producer_max);
gpf_status summarize(gpf_filter* h, const PrioView& pv, WSum* slot, const ScanRequest& rq, bool* published = nullptr);   // *published: this scan publishes its summary itself (read_published_summary)
gpf_status ensure_raw(gpf_filter* h, bool want_q = false, bool* published = nullptr);
gpf_status ensure_raw_summary(gpf_filter* h, bool want_q, bool* done);
gpf_status read_published_summary(gpf_filter* h, WSum& w);
bool sum_host_ok(const gpf_filter* h);
gpf_status sum_host_launch(gpf_filter* h, const double* thr);
gpf_status sum_host_fold(gpf_filter* h, const double* thr, int* go_out = nullptr);
gpf_status sum_gate_check(gpf_filter* h, int host_go, int64_t ticket);
gpf_status shard_sum_launch(gpf_filter* h, const ShardSum& ss, bool* ok);
bool shard_sum_collect();                                        // GPF_SHARD_SUM=collect: k_sum_reduce<SHARD> instead of k_sum_shard
gpf_status check_scan_timeout(gpf_filter* h);
gpf_status fetch_scalars(gpf_filter* h, bool fold_raw_q = false);
gpf_status sort_desc(gpf_filter* h, const PrioView& pv, int64_t n);
gpf_status ensure_residual_buffers(gpf_filter* h);
CdfLevels levels(const gpf_filter* h, int ch);
gpf_status residual_scans(gpf_filter* h, const WSum* ws, int64_t n_slots_global, int32_t* head_anc = nullptr, const ResidDirect* direct = nullptr);
void launch_multinomial_search(gpf_filter* h, const SearchArgs& sa);
void launch_search_plain(gpf_filter* h, int which, int grid, size_t lds, const SearchArgs& sa);   // k_search<which>, which = 1 (residual) | 3 (systematic)
void launch_search_strat(gpf_filter* h, const SearchArgs& sa, int64_t n_slots, bool sorted_uniforms);   // k_search_strat<sorted_uniforms>
gpf_status sorted_job_prepare(gpf_filter* h, int64_t gid0, int64_t n_slots);
gpf_status sorted_gammas_finish(gpf_filter* h, bool with_tiles, bool gammas_pending);
gpf_status finish_search(gpf_filter* h);
gpf_status resample_impl(gpf_filter* h, int method, PrioView pv, int sort_particles, int check, int32_t* invalid, bool local = false);
// a block of <= 128 / <= 512 particles is the work of one wave (2 / 8 particles per lane, BLOCK / WAVE blocks per workgroup), a larger one of a workgroup:
// f(TEAM, ITEMS, grid) with TEAM and ITEMS as std::integral_constant -- the template arguments of the block kernels (gpf_k_block.hpp) -- and their grid
template <class F>
inline void team_dispatch(int64_t block_size, int64_t nblocks, F&& f)
{
    constexpr int TEAMS = BLOCK / WAVE;                          // wave teams of a workgroup
    const dim3 waves((unsigned)((nblocks + TEAMS - 1) / TEAMS)), groups((unsigned)nblocks);
    if (block_size <= 2 * WAVE)      f(std::integral_constant<int, WAVE>{}, std::integral_constant<int, 2>{}, waves);
    else if (block_size <= 8 * WAVE) f(std::integral_constant<int, WAVE>{}, std::integral_constant<int, 8>{}, waves);
    else                             f(std::integral_constant<int, BLOCK>{}, std::integral_constant<int, 8>{}, groups);
}
// ---- defined in libgpf_aux.hip
gpf_status weighted_tree_sum(gpf_filter* h, const double* values, int stride, int col, int pw, const double* center, double match, double* out_dev);
// the per-particle kernels of the block-wise initialise / propagate / move (called from libgpf_blocks.hip): k_init / k_step / k_move<model, ...> by the
// handle's keep_prev and per-block parameters; mode 0 | 2 | MODE_REF, the propagate 4 as well
void launch_init_blk(gpf_filter* h, int grid, int mode);
void launch_step_blk(gpf_filter* h, int grid, int mode);
void launch_move_blk(gpf_filter* h, int grid, int n_iters, bool reweight);
// ---- defined in libgpf_blocks.hip: what the block-wise filter shares with the store's queries (libgpf_store.hip) and the forward smoother (libgpf_forward.hip)
// The preconditions of a block-wise call, in ONE order for every entry point ("the gate of the block-wise calls"); `steps` names the ones
// the entry point has.  Nothing here touches the handle -- check_ready, which brings a lazy move or a view up to date, comes after the gate and after the
// entry point's own checks -- so a refused call changes nothing.  The null handle is refused always.
enum : unsigned {
    GATE_VIEW = 1, GATE_SHARD = 2,
    GATE_STORE = 4,            // a filter with the plain trajectory store (gpf_history_enable) takes no block-wise call
    GATE_STORE_VIEWS = 8,      //   ... and says why: the estimates of big blocks are the work of sub-state views, which it does not have
    GATE_SIZE = 16,            // block_size < 1
    GATE_CLAMP = 32,           // block_size comes back clamped to the particle count: "one block" may be asked for as any size >= n, 2^32 included (the
                               // step kernels divide by it as a 32-bit number, ModelArgs::blk_size, and n < 2^31)
    GATE_CLAMP_STORE = 64,     //   ... only on a filter with the block-wise store (elsewhere a size >= n stays what it is: above BLK_MAX the work of a view)
    GATE_MAX = 128,            // blocks of more than BLK_MAX particles are the work of view handles (big_block_views), which a filter with the block-wise store
                               // (gpf_history_enable_blocks) does not have
    GATE_PARAMS = 256,         // the block size of the per-block parameters, where they are set
    GATE_FWD = 512,            // the block size of forward smoothing per block (gpf_forward_enable_blocks), once its initialising call has set it
    GATE_FILTER = GATE_VIEW | GATE_SHARD | GATE_STORE | GATE_SIZE,
};
gpf_status block_gate(gpf_handle h, int64_t& block_size, const char* who, unsigned steps);
// the results of a call from the device to the host, each where the caller wants it (nullptr: not asked for), then the one synchronisation
struct OutCopy { const void* dev; void* host; size_t bytes; };
gpf_status block_out(gpf_filter* h, std::initializer_list<OutCopy> outs);
// the parameters a transition density is evaluated with: the filter's own, and the per-block rows where they are set
AncArgs anc_args(const gpf_filter* h);
// the device buffer of the per-block estimates (h->blk_est): at least `need` doubles
gpf_status block_est_buffer(gpf_filter* h, int64_t need);
// the match values of a proportion kernel, padded with the last one (the kernels take them two at a time)
BlockMatch make_block_match(const double* values, int32_t n_values);
// ---- defined in libgpf_smooth.hip
void launch_block_smooth(gpf_filter* h, const SmoothArgs& a, const AncArgs& x);   // k_block_smooth<model, TEAM, ITEMS> by team_dispatch
// ---- defined in libgpf_pairs.hip
void launch_block_pairs(gpf_filter* h, const PairArgs& a, const AncArgs& x);      // k_block_smooth_pairs<model, TEAM, ITEMS> by team_dispatch
// ---- defined in libgpf_map.hip
void launch_block_map(gpf_filter* h, const MapArgs& a, const AncArgs& x);         // k_block_map<model, TEAM, ITEMS> by team_dispatch
// ---- defined in libgpf_run.hip
void launch_block_run(gpf_filter* h, const RunArgs& a, int method);               // k_block_run<model, W, method, TEAM, ITEMS> by team_dispatch; method 0 | 1 | 2
// ---- defined in libgpf_forward.hip: the forward-only smoother's records (hist_begin_step / hist_on_resample call the first two) and launches
gpf_status fwd_begin_step(gpf_filter* h, bool first);             // first: step 1 begins, the statistics are reset; else the step that ends is closed in its final order
gpf_status fwd_on_resample(gpf_filter* h, int64_t block_size);    // this call's parents into the current step's map (block_size > 0: block-local, h->blk_mask says which)
gpf_status fwd_form(gpf_filter* h);                               // k_block_forward<model>: the current step's statistics into fwd_T[1 - fwd_cur]; nothing is committed
void launch_block_forward_reduce(gpf_filter* h, const double* T, double* out);   // k_block_forward_reduce<d, TEAM, ITEMS> by team_dispatch
void fwd_free(gpf_filter* h);
// ---- defined in libgpf_shard.hip
gpf_status shard_device_setup(gpf_filter* h);         // LDS attributes of the push kernels (gpf_create)

} // namespace gpfh
