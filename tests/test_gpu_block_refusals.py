"""The preconditions of the block-wise entry points (gpf.h), pinned call by call: status and the full gpf_last_error text.

Every block-wise call passes one gate, in this order: 1 null handle, 2 sub-state view, 3 shard, 4 plain trajectory store, 5 block_size < 1, 6 the clamp
to the particle count, 7 the block-wise store and more than 2048 particles per block, 8 agreement with the per-block parameters (the
block-wise section).  Which steps an entry point has is its own business; STEPS below names them.  The queries of the block-wise store go on in one
order of their own: steps 5-7, "needs the block-wise trajectory store", [the two that read weight records: "needs the store's weight records", step 8],
the query's own arguments, the filter brought up to date, the step range, [the 2^31 limits], [the block size every walked step was entered with].

  test_single_refusals        every entry point against every step it has, ONE fault at a time, and its null-handle call.
  test_store_query_arguments  the five store queries against what comes behind their gate, ONE fault at a time.
  test_refusal_order          two refusals at once, or one refusal on a filter that is not initialised: the earlier step of the orders above is reported,
                              and the filter is not brought up to date first.  Nothing else about simultaneous faults is asserted anywhere."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INVALID_ARGUMENT, STATE = 1, 6                                               # gpf_status
NAN = float("nan")

VIEW = " on a sub-state view: call it on the filter"
SHARD = " on a shard of a sharded filter"
STORE = " on a filter with a trajectory store"
STORE_VIEWS = " on a filter with a trajectory store (it has no sub-state views)"
SIZE = "block_size < 1"
MAX = ": blocks of more than 2048 particles on a filter with a trajectory store (they would need sub-state views)"
PARAMS = ": block_size 50 differs from the 100 of the per-block parameters (gpf_set_block_params)"
NEEDS_STORE = " needs the block-wise trajectory store (gpf_history_enable_blocks before gpf_initialize_blocks)"
NEEDS_WEIGHTS = " needs the store's weight records (gpf_history_enable_blocks_weights before gpf_initialize_blocks)"
RANGE = ": need 1 <= step_lo <= step_hi <= gpf_history_steps"
DRAWS = ": n_blocks * n_samples and n_blocks * n_samples * n_steps * dim must stay below 2^31"
ENTERED_SIZE = ": block_size 50 differs from the 100 step 2 was entered with"
ENTERED_WHOLE = ": step 2 was entered by a whole-filter call (no per-block observations were recorded)"

STEP_FAMILY = ["gpf_initialize_blocks", "gpf_update_blocks", "gpf_initialize_blocks_ref", "gpf_update_blocks_ref", "gpf_initialize_blocks_strata",
               "gpf_update_blocks_strata", "gpf_update_blocks_proposal"]
WEIGHT_QUERIES = ["gpf_block_backward_sample", "gpf_block_smooth"]             # the store queries that read the store's weight records
STORE_QUERIES = ["gpf_block_history_moments", "gpf_block_history_proportion", "gpf_block_sample_trajectories"] + WEIGHT_QUERIES
# the steps 2-8 of every entry point (step 1, the null handle, all of them have; gpf_rejuvenate_blocks takes its block size from the handle: below)
STEPS = {"gpf_resample_blocks": "23457", "gpf_resample_blocks_conditional": "2345", "gpf_block_stats": "2357", "gpf_block_moments": "23457",
         "gpf_block_proportion": "23457", "gpf_set_block_params": "2345", "gpf_get_block_params": "2", "gpf_resample_across_blocks": "234578",
         "gpf_rejuvenate_blocks": "", "gpf_resample_blocks_ancestor": "23458", "gpf_block_ancestor_log_weights": "2345"}
STEPS.update({w: "23458" for w in STEP_FAMILY})
STEPS.update({w: "57" for w in STORE_QUERIES})
STEPS.update({w: "578" for w in WEIGHT_QUERIES})                             # (step 8 behind their store and weight-record refusals)


def pd(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


@pytest.fixture(scope="module")
def world(g):
    """the handles of the issue and one caller per entry point: call[who](handle, block_size) -> status, every other argument valid"""
    m = g.models.lgssm2()
    y = np.ascontiguousarray(g.models.simulate(m, 1)[0], np.float64)
    n_obs, n_par = y.size, len(m.params)
    obs = np.ascontiguousarray(np.tile(y, (4200, 1)))                        # (more rows than any call has blocks)
    buf = np.zeros(4200 * 8)
    ibuf = np.zeros(4200, np.int32)
    vals = np.array([0.0, 1.0])
    par = np.ascontiguousarray(np.tile(np.asarray(m.params, np.float64), (4200, 1)))
    L = g._lib.load()
    H = {}
    H["plain"] = g.pf_initialize(m, (1,), y, 300, seed=3)
    H["view"] = H["plain"][0:100]
    H["shard"] = g.DeviceParticleFilterState(m, 100, seed=1, n_global=200, gid0=0)
    assert L.gpf_initialize(H["shard"]._h, pd(y), n_obs) == 0
    H["store"] = g.pf_initialize(m, (1,), y, 300, seed=3, history=4)
    H["bstore"] = g.pf_initialize_blocks(m, (1,), obs[:42], 4200, 100, seed=3, history=2)
    H["bp"] = g.pf_initialize(m, (1,), y, 300, seed=3)
    assert L.gpf_set_block_params(H["bp"]._h, pd(par), n_par, 100) == 0
    H["uninit"] = g.DeviceParticleFilterState(m, 300, seed=3)
    # per-block observations at size 100, per-block parameters at size 50: what gpf_rejuvenate_blocks refuses
    H["moved"] = g.pf_initialize_blocks(m, (1,), obs[:3], 300, 100, seed=3, keep_prev=True)
    assert L.gpf_set_block_params(H["moved"]._h, pd(par), n_par, 50) == 0
    # bstore with weight records and a second step (T = 2); the same with per-block parameters at the steps' block size
    for k in ("wstore", "wbp"):
        H[k] = g.pf_initialize_blocks(m, (1,), obs[:42], 4200, 100, seed=3, history=2, history_weights=True)
        g.pf_update_blocks(H[k], (2,), (None,), obs[:42], 100)
    assert L.gpf_set_block_params(H["wbp"]._h, pd(par), n_par, 100) == 0
    # bstore with per-block parameters: no weight records AND a block size the parameters refuse
    H["bstore_bp"] = g.pf_initialize_blocks(m, (1,), obs[:42], 4200, 100, seed=3, history=2)
    assert L.gpf_set_block_params(H["bstore_bp"]._h, pd(par), n_par, 100) == 0
    # a store with weight records whose step 2 was entered by a whole-filter pf_update, a whole-filter resample behind it
    H["wwhole"] = g.pf_initialize_blocks(m, (1,), obs[:3], 300, 100, seed=3, history=2, history_weights=True)
    g.pf_update(H["wwhole"], (2,), (None,), y)
    g.pf_resample(H["wwhole"], "multinomial")
    H["wuninit"] = g.DeviceParticleFilterState(m, 300, seed=3, history=2, history_blocks=True, history_weights=True)
    pi = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
    lbuf = np.zeros(4200 * 2, np.int64)
    call = {
        "gpf_resample_blocks": lambda h, bs, method=0: L.gpf_resample_blocks(h, method, bs, NAN, 0, NAN, 0, None, None),
        "gpf_resample_blocks_conditional": lambda h, bs, method=0: L.gpf_resample_blocks_conditional(h, method, bs, NAN, 0, None, None),
        "gpf_block_stats": lambda h, bs: L.gpf_block_stats(h, bs, pd(buf), pd(buf)),
        "gpf_block_moments": lambda h, bs, out=pd(buf): L.gpf_block_moments(h, bs, out, out),
        "gpf_block_proportion": lambda h, bs: L.gpf_block_proportion(h, bs, 0, pd(vals), 1, pd(buf)),
        "gpf_initialize_blocks": lambda h, bs: L.gpf_initialize_blocks(h, pd(obs), n_obs, bs),
        "gpf_update_blocks": lambda h, bs: L.gpf_update_blocks(h, pd(obs), n_obs, bs),
        "gpf_initialize_blocks_ref": lambda h, bs: L.gpf_initialize_blocks_ref(h, pd(obs), n_obs, bs, pd(buf), m.dim),
        "gpf_update_blocks_ref": lambda h, bs: L.gpf_update_blocks_ref(h, pd(obs), n_obs, bs, pd(buf), m.dim),
        "gpf_initialize_blocks_strata": lambda h, bs: L.gpf_initialize_blocks_strata(h, pd(obs), n_obs, bs, pd(vals), 2, 0),
        "gpf_update_blocks_strata": lambda h, bs: L.gpf_update_blocks_strata(h, pd(obs), n_obs, bs, pd(vals), 2, 0),
        "gpf_update_blocks_proposal": lambda h, bs: L.gpf_update_blocks_proposal(h, pd(obs), n_obs, bs, ibuf.ctypes.data_as(C.POINTER(C.c_int32)), 0),
        "gpf_rejuvenate_blocks": lambda h, bs=None: L.gpf_rejuvenate_blocks(h, 0, 1, 0, None),
        "gpf_set_block_params": lambda h, bs, n=n_par: L.gpf_set_block_params(h, pd(par), n, bs),
        "gpf_get_block_params": lambda h, bs: L.gpf_get_block_params(h, pd(buf), n_par, 3),
        "gpf_resample_across_blocks": lambda h, bs: L.gpf_resample_across_blocks(h, 0, bs, 0, NAN, 0, None, None, None),
        "gpf_block_history_moments": lambda h, bs, step=1: L.gpf_block_history_moments(h, step, bs, pd(buf), pd(buf)),
        "gpf_block_history_proportion": lambda h, bs: L.gpf_block_history_proportion(h, 1, bs, 0, pd(vals), 1, pd(buf)),
        "gpf_block_sample_trajectories": lambda h, bs, k=1, lo=1, hi=1, out=True:
            L.gpf_block_sample_trajectories(h, bs, k, lo, hi, pd(buf) if out else None, pi(lbuf) if out else None),
        "gpf_block_backward_sample": lambda h, bs, k=1, lo=1, hi=1, out=True:
            L.gpf_block_backward_sample(h, bs, k, lo, hi, pd(buf) if out else None, pi(lbuf) if out else None),
        "gpf_block_smooth": lambda h, bs, lo=1, hi=1, out=True: L.gpf_block_smooth(h, bs, lo, hi, pd(buf) if out else None, None, None, None),
        "gpf_resample_blocks_ancestor": lambda h, bs: L.gpf_resample_blocks_ancestor(h, 0, bs, NAN, 0, pd(obs), n_obs, pd(buf), m.dim, None, None),
        "gpf_block_ancestor_log_weights": lambda h, bs: L.gpf_block_ancestor_log_weights(h, bs, pd(obs), n_obs, pd(buf), m.dim, pd(buf)),
    }
    assert set(call) == set(STEPS)
    yield L, H, call
    for k in ("view", "plain", "shard", "store", "bstore", "bp", "uninit", "moved", "wstore", "wbp", "bstore_bp", "wwhole", "wuninit"):
        H[k].close()


def answer(L, h, status):
    return status, L.gpf_last_error(h).decode()


def test_single_refusals(world):
    L, H, call = world
    h = {k: v._h for k, v in H.items()}
    for who, steps in STEPS.items():
        f = call[who]
        assert answer(L, None, f(None, 100)) == (INVALID_ARGUMENT, "null handle"), who
        if "2" in steps:
            assert answer(L, h["view"], f(h["view"], 50)) == (STATE, who + VIEW), who
        if "3" in steps:
            assert answer(L, h["shard"], f(h["shard"], 50)) == (STATE, who + SHARD), who
        if "4" in steps:
            text = who + (STORE_VIEWS if who in ("gpf_block_moments", "gpf_block_proportion") else STORE)
            assert answer(L, h["store"], f(h["store"], 100)) == (STATE, text), who
        if "5" in steps:
            on = "bstore" if who in STORE_QUERIES else "plain"
            assert answer(L, h[on], f(h[on], 0)) == (INVALID_ARGUMENT, SIZE), who
            assert answer(L, h[on], f(h[on], -7)) == (INVALID_ARGUMENT, SIZE), who
        if "7" in steps:
            assert answer(L, h["bstore"], f(h["bstore"], 2100)) == (STATE, who + MAX), who
        if "8" in steps:
            on = "wbp" if who in WEIGHT_QUERIES else "bp"
            assert answer(L, h[on], f(h[on], 50)) == (INVALID_ARGUMENT, who + PARAMS), who
    # the block size of gpf_rejuvenate_blocks is that of the per-block observations
    assert answer(L, h["moved"], call["gpf_rejuvenate_blocks"](h["moved"])) == \
        (INVALID_ARGUMENT, "gpf_rejuvenate_blocks: block_size 100 differs from the 50 of the per-block parameters (gpf_set_block_params)")
    # the store queries on a filter without the block-wise store
    for who in STORE_QUERIES:
        for on in ("plain", "store"):
            assert answer(L, h[on], call[who](h[on], 100)) == (STATE, who + NEEDS_STORE), (who, on)
    # where the conditional resample would reach step 7 it has a refusal of its own
    assert answer(L, h["bstore"], call["gpf_resample_blocks_conditional"](h["bstore"], 2100)) == \
        (INVALID_ARGUMENT, "gpf_resample_blocks_conditional: blocks of more than 2048 particles resample through sub-state views, which have no conditional form")
    # and the calls go through where nothing is wrong
    assert call["gpf_block_stats"](h["plain"], 100) == 0 and call["gpf_block_moments"](h["bstore"], 2048) == 0
    assert call["gpf_get_block_params"](h["bp"], 100) == 0


def test_store_query_arguments(world):
    """the five queries of the block-wise store behind their gate: the refusals of their own arguments, ONE fault at a time, on a store of T = 2 steps"""
    L, H, call = world
    h = {k: v._h for k, v in H.items()}
    w, b = h["wstore"], h["bstore"]
    vals17 = np.zeros(17)
    walkers = ["gpf_block_sample_trajectories"] + WEIGHT_QUERIES
    samplers = ["gpf_block_sample_trajectories", "gpf_block_backward_sample"]
    # outputs all NULL
    assert answer(L, w, L.gpf_block_history_moments(w, 1, 100, None, None)) == (INVALID_ARGUMENT, "gpf_block_history_moments: both outputs are NULL")
    assert answer(L, w, L.gpf_block_history_proportion(w, 1, 100, 0, pd(vals17), 1, None)) == (INVALID_ARGUMENT, "gpf_block_history_proportion: null values / output")
    for who, text in zip(walkers, (": both outputs are NULL", ": null trajectory output", ": all outputs are NULL")):
        assert answer(L, w, call[who](w, 100, out=False)) == (INVALID_ARGUMENT, who + text), who
    for who in samplers:
        # n_samples < 1; the 2^31 limit (refused before anything is allocated)
        for k in (0, -3):
            assert answer(L, w, call[who](w, 100, k)) == (INVALID_ARGUMENT, who + ": n_samples < 1"), who
        assert answer(L, w, call[who](w, 100, 2 ** 31 - 1, 1, 2)) == (INVALID_ARGUMENT, who + DRAWS), who
    for who in walkers:
        # the three bad step ranges
        for lo, hi in ((0, 2), (2, 1), (1, 3)):
            assert answer(L, w, call[who](w, 100, lo=lo, hi=hi)) == (INVALID_ARGUMENT, who + RANGE), (who, lo, hi)
    for who in WEIGHT_QUERIES:
        # a store without weight records; another block size than the walked step was entered with; a walked step entered by a whole-filter pf_update
        assert answer(L, b, call[who](b, 100)) == (STATE, who + NEEDS_WEIGHTS), who
        assert answer(L, w, call[who](w, 50, lo=1, hi=2)) == (INVALID_ARGUMENT, who + ENTERED_SIZE), who
        assert answer(L, h["wwhole"], call[who](h["wwhole"], 100, lo=1, hi=2)) == (STATE, who + ENTERED_WHOLE), who
    # the history proportion's column and number of values; the step of both history estimates
    for col in (-1, 2):
        assert answer(L, w, L.gpf_block_history_proportion(w, 1, 100, col, pd(vals17), 1, pd(vals17))) == (INVALID_ARGUMENT, "bad column"), col
    for k in (0, 17):
        assert answer(L, w, L.gpf_block_history_proportion(w, 1, 100, 0, pd(vals17), k, pd(vals17))) == \
            (INVALID_ARGUMENT, "gpf_block_history_proportion: need 1 <= n_values <= 16"), k
    buf = np.zeros(42 * 16)
    for step in (0, -1, 3):
        assert answer(L, w, L.gpf_block_history_moments(w, step, 100, pd(buf), pd(buf))) == (INVALID_ARGUMENT, "bad step"), step
        assert answer(L, w, L.gpf_block_history_proportion(w, step, 100, 0, pd(vals17), 1, pd(buf))) == (INVALID_ARGUMENT, "bad step"), step
    # and the calls go through where nothing is wrong
    for who in walkers:
        assert call[who](w, 100, lo=1, hi=2) == 0, who
    assert L.gpf_block_history_moments(w, 2, 100, pd(buf), pd(buf)) == 0 and L.gpf_block_history_proportion(w, 1, 100, 0, pd(vals17), 16, pd(buf)) == 0


def test_refusal_order(world):
    L, H, call = world
    h = {k: v._h for k, v in H.items()}
    # a filter that is not initialised and a bad block size: the block size is refused, the filter is not looked at
    for who in ("gpf_resample_blocks", "gpf_block_stats"):
        assert answer(L, h["uninit"], call[who](h["uninit"], 0)) == (INVALID_ARGUMENT, SIZE), who
    # the gate comes before the checks an entry point has of its own
    for who in ("gpf_resample_blocks", "gpf_resample_blocks_conditional"):   # (an unknown method, a method without a conditional form)
        assert answer(L, h["store"], call[who](h["store"], 100, 1 if "cond" in who else 7)) == (STATE, who + STORE), who
    assert answer(L, h["view"], call["gpf_block_moments"](h["view"], 50, None)) == (STATE, "gpf_block_moments" + VIEW)
    assert answer(L, h["bp"], call["gpf_resample_across_blocks"](h["bp"], 70)) == \
        (INVALID_ARGUMENT, "gpf_resample_across_blocks: block_size 70 differs from the 100 of the per-block parameters (gpf_set_block_params)")
    assert answer(L, h["bstore"], call["gpf_block_sample_trajectories"](h["bstore"], 0, 0)) == (INVALID_ARGUMENT, SIZE)
    assert answer(L, h["bstore"], call["gpf_block_history_moments"](h["bstore"], 2100, 99)) == (STATE, "gpf_block_history_moments" + MAX)
    assert answer(L, h["plain"], call["gpf_set_block_params"](h["plain"], 0, 0)) == (INVALID_ARGUMENT, SIZE)
    for who in WEIGHT_QUERIES:
        # no weight records and a block size the per-block parameters refuse: the weight records come first
        assert answer(L, h["bstore_bp"], call[who](h["bstore_bp"], 50)) == (STATE, who + NEEDS_WEIGHTS), who
    for who in ["gpf_block_sample_trajectories"] + WEIGHT_QUERIES:
        # a bad step range behind a whole-filter resample (whatever it left deferred; a lazy move is never pending here -- gpf_rejuvenate keeps none on
        # a filter with a trajectory store): refused with the range text.  On a filter that is not initialised the range is not looked at
        assert answer(L, h["wwhole"], call[who](h["wwhole"], 100, lo=2, hi=3)) == (INVALID_ARGUMENT, who + RANGE), who
        assert answer(L, h["wuninit"], call[who](h["wuninit"], 100, lo=2, hi=3)) == \
            (STATE, "filter not initialised: call gpf_initialize (pf_initialize) first"), who
