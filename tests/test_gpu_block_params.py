"""Per-block model parameters (gpf.h gpf_set_block_params): many parameter values in one state.  Block b of the device state must equal, bit for
bit, block b of an oracle filter created with block b's parameters -- the reference's loop over sub-states with per-view arguments (src/update.jl:
12-25 on a sub-state, src/view.jl:35-48), built in tests/block_params_spec.py from the existing oracle block helpers -- and block b of a device
filter created with those parameters under the shared-parameter block calls.  Refusals leave the state bit-identical."""
import numpy as np
import pytest

import block_params_spec as sp
from conftest import soak_grid

pytestmark = pytest.mark.gpu

PARAM_SETS = {                                             # K = 3 distinct parameter vectors per model
    "lgssm2": lambda m: [m.lgssm2(rho=0.9, sr=0.3), m.lgssm2(rho=0.99, sr=0.8, theta=0.3), m.lgssm2(sq=0.3, s0=2.0)],
    "sv1": lambda m: [m.sv1(), m.sv1(mu=0.5, phi=0.8, sigma=0.4), m.sv1(mu=-2.0, phi=0.99, sigma=0.05)],
    "bearings4": lambda m: [m.bearings4(), m.bearings4(sb=0.02, sp=0.003), m.bearings4(sv=0.004, sb=0.01)],
    "object_motion": lambda m: [m.object_motion(), m.object_motion(p_stay=0.95, p_start=0.05, sobs=0.5), m.object_motion(sy=0.2)],
}


def assignment(B):
    return (np.arange(B) * np.arange(B) + np.arange(B) // 2) % 3          # every set, in no regular pattern


def block_obs(g, m, B, T, seed=7):
    base = np.asarray(g.models.simulate(m, T))
    return base[None, :, :] + 0.3 * np.random.default_rng(seed).standard_normal((B,) + base.shape)


def snapshot(g, st):
    return st.traces.copy(), st.log_weights.copy(), st.parents.copy(), g.get_lml_est(st)


def same_state(st, ref):
    return np.array_equal(st.traces, ref.rows) and np.array_equal(st.log_weights, ref.lw) and np.array_equal(st.parents, ref.parents)


def setup(g, o, model_name, N, nb, seed=13, T=5):
    m = g.models.by_name(model_name)
    sets = PARAM_SETS[model_name](g.models)
    B = (N + nb - 1) // nb
    assign = assignment(B)
    ys = block_obs(g, m, B, T)
    st = g.pf_initialize_blocks(m, (1,), ys[:, 0], N, nb, seed=seed, keep_prev=True, params=[sets[k] for k in assign])
    ref = sp.ParamBlocksOracle(o, m.model_id, [s.params for s in sets], assign, N, nb, seed, keep_prev=True).initialize(ys[:, 0])
    return m, sets, assign, ys, st, ref


def _keep(model_name, nb):
    return (model_name, nb) in {("lgssm2", 100), ("bearings4", 64), ("sv1", 513), ("lgssm2", 2500)}


@pytest.mark.parametrize("model_name,nb", soak_grid(["lgssm2", "sv1", "bearings4"], [1, 7, 64, 100, 129, 513, 2048, 2500], keep=_keep))
def test_reference_loop_bit_for_bit(g, o, model_name, nb):
    """init -> (update -> ESS-triggered residual resample -> move / reweight, with and without only_resampled) x T -> the whole-filter
    pf_rejuvenate after the block update: rows, weights, parents, accept counts and block_stats equal the K oracle filters block by block"""
    N = min(5 * nb + nb // 2 + 1, 13000) if nb > 1 else 37
    T = 5
    m, sets, assign, ys, st, ref = setup(g, o, model_name, N, nb, T=T)
    assert same_state(st, ref), "initialize"
    for t in range(1, T):
        g.pf_update_blocks(st, (t + 1,), (None,), ys[:, t], nb); ref.update(ys[:, t])
        assert same_state(st, ref), ("update", t)
        n_res = g.pf_resample_blocks(st, nb, "residual", ess_frac=0.5, check=False)
        mask = ref.resample("residual", ess_frac=0.5)
        assert n_res == mask.sum() and same_state(st, ref), ("resample", t)
        method = "move" if t % 2 else "reweight"
        only = t % 3 != 0
        acc = g.pf_rejuvenate_blocks(st, None, (), 1, method=method, only_resampled=only, count=True)
        assert acc == ref.rejuvenate(ys[:, t], method, mask=mask if only else None), ("accepts", t)
        assert same_state(st, ref), ("rejuvenate", method, only, t)
    ess, lml = g.block_stats(st, nb)
    assert np.array_equal(lml, ref.block_lml()) and np.array_equal(ess, ref.block_ess())
    g.pf_rejuvenate(st, None, (), 1, method="move"); ref.rejuvenate(ys[:, T - 1], "move")
    assert same_state(st, ref), "whole-filter pf_rejuvenate after the block update"
    st.close()


@pytest.mark.parametrize("nb", [100, 7])
def test_proposal_blocks(g, o, nb):
    """gpf_update_blocks_proposal with lgssm2: the locally optimal proposal's constants (gain, sv, ...) are the block's own"""
    N, T = 6 * nb + 3, 5
    m, sets, assign, ys, st, ref = setup(g, o, "lgssm2", N, nb, T=T)
    B = assign.size
    for t in range(1, T):
        flags = (np.arange(B) + t) % 3 != 0
        g.pf_update_blocks(st, (t + 1,), (None,), ys[:, t], nb, proposals=[g.locally_optimal if f else None for f in flags])
        ref.update(ys[:, t], proposals=flags)
        assert same_state(st, ref), t
        g.pf_resample_blocks(st, nb, "multinomial", ess_frac=0.6, check=False); ref.resample("multinomial", ess_frac=0.6)
        assert same_state(st, ref), t
    assert np.array_equal(g.block_stats(st, nb)[1], ref.block_lml())
    st.close()


@pytest.mark.parametrize("layout", ["contiguous", "interleaved"])
def test_strata_blocks(g, o, layout):
    """gpf_{initialize,update}_blocks_strata with object_motion: p(moving) and log p of the constrained latent are the block's own"""
    N, nb, T = 1030, 100, 4
    m = g.models.object_motion()
    sets = PARAM_SETS["object_motion"](g.models)
    B = (N + nb - 1) // nb
    assign = assignment(B)
    ys = block_obs(g, m, B, T)
    st = g.pf_initialize_blocks(m, (1,), ys[:, 0], N, nb, seed=13, keep_prev=True, strata=[0.0, 1.0], layout=layout, params=[sets[k] for k in assign])
    ref = sp.ParamBlocksOracle(o, m.model_id, [s.params for s in sets], assign, N, nb, 13).initialize(ys[:, 0], strata=[0.0, 1.0], layout=layout)
    assert same_state(st, ref)
    for t in range(1, T):
        g.pf_update_blocks(st, (t + 1,), (None,), ys[:, t], nb, strata=[0.0, 1.0], layout=layout)
        ref.update(ys[:, t], strata=[0.0, 1.0], layout=layout)
        assert same_state(st, ref), t
        g.pf_resample_blocks(st, nb, "stratified", ess_frac=0.9, check=False); ref.resample("stratified", ess_frac=0.9)
        assert same_state(st, ref), t
    st.close()


def test_device_vs_device(g, o):
    """block b equals block b of a device filter created with params = row b, run through the shared-parameter block calls"""
    N, nb, T = 1000, 100, 4
    m, sets, assign, ys, st, _ = setup(g, o, "bearings4", N, nb, T=T)
    twins = [g.pf_initialize_blocks(s, (1,), ys[:, 0], N, nb, seed=13, keep_prev=True) for s in sets]
    for t in range(1, T):
        for x in [st] + twins:
            g.pf_update_blocks(x, (t + 1,), (None,), ys[:, t], nb)
            g.pf_resample_blocks(x, nb, "residual", ess_frac=0.5, check=False)
            g.pf_rejuvenate_blocks(x, None, (), 1, method="move" if t % 2 else "reweight", only_resampled=True)
    rows, lw, par = st.traces, st.log_weights, st.parents
    lml = g.block_stats(st, nb)[1]
    tw = [(x.traces, x.log_weights, x.parents, g.block_stats(x, nb)[1]) for x in twins]
    for b in range(assign.size):
        sl = slice(b * nb, min((b + 1) * nb, N))
        r, w, p, l = tw[assign[b]]
        assert np.array_equal(rows[sl], r[sl]) and np.array_equal(lw[sl], w[sl]) and np.array_equal(par[sl], p[sl]) and lml[b] == l[b], b
    for x in [st] + twins:
        x.close()


def test_refusals_leave_the_state_alone(g, o):
    N, nb = 600, 100
    m, sets, assign, ys, st, ref = setup(g, o, "lgssm2", N, nb)
    g.pf_update_blocks(st, (2,), (None,), ys[:, 1], nb); ref.update(ys[:, 1])
    before = snapshot(g, st)
    L, h = st._L, st._h
    pd = g.api._pd
    o1 = np.ascontiguousarray(ys[0, 0]); strata = np.array([0.0, 1.0])
    refused = {
        "update": lambda: L.gpf_update(h, o1.ctypes.data, 2),
        "update_proposal": lambda: L.gpf_update_proposal(h, pd(o1), 2, 1),
        "initialize": lambda: L.gpf_initialize(h, pd(o1), 2),
        "initialize_proposal": lambda: L.gpf_initialize_proposal(h, pd(o1), 2, 1),
        "step_ess": lambda: L.gpf_step_ess(h, o1.ctypes.data, 2, 0.5, 1, 0, 0, -1, 0, None, None, None),
        "introduce": lambda: L.gpf_introduce(h, pd(o1), 2, 1, 10, 0),
        "resize": lambda: L.gpf_resize(h, 500, 0, float("nan"), 0, None),
        "replicate": lambda: L.gpf_replicate(h, 2, 0),
        "dereplicate": lambda: L.gpf_dereplicate(h, 2, 0, 0),
        "coalesce": lambda: L.gpf_coalesce(h, 0, None),
        "rejuvenate_with_proposal": lambda: L.gpf_rejuvenate_with_proposal(h, 1, 1, None, 0, 1, None),
    }
    for name, call in refused.items():
        assert call() == g._lib.ERR_STATE, name
        assert "per-block model parameters" in L.gpf_last_error(h).decode(), name
    # a different block size: GPF_ERR_INVALID_ARGUMENT, nothing changes
    with pytest.raises(g.ErrorException, match="differs"):
        g.pf_update_blocks(st, (3,), (None,), np.tile(ys[0, 2], (12, 1)), 50)
    # model-dependent calls on a view of the filter
    v = st[0:100]
    with pytest.raises(g.ErrorException, match="per-block model parameters"):
        g.pf_update(v, (3,), (None,), ys[0, 2])
    with pytest.raises(g.ErrorException, match="per-block model parameters"):
        g.pf_rejuvenate(v, None, (), 1)
    # the setter on a view, a shard, a filter with a trajectory store; bad shapes
    with pytest.raises(g.ErrorException, match="view"):
        g.set_block_params(v, [sets[0]], 100)
    for a, b in zip(snapshot(g, st)[:3], before[:3]):
        assert np.array_equal(a, b)
    assert snapshot(g, st)[3] == before[3]
    shard = g.DeviceParticleFilterState(m, 100, seed=1, n_global=200, gid0=0)
    with pytest.raises(g.ErrorException, match="shard"):
        g.set_block_params(shard, [sets[0]], 100)
    hist = g.DeviceParticleFilterState(m, 100, seed=1, history=4)
    with pytest.raises(g.ErrorException, match="trajectory"):
        g.set_block_params(hist, [sets[0]], 100)
    rows = np.stack([s.params for s in sets])
    assert L.gpf_set_block_params(h, pd(np.ascontiguousarray(rows)), 25, 100) == g._lib.ERR_INVALID_ARGUMENT
    assert L.gpf_set_block_params(h, pd(np.ascontiguousarray(rows)), 20, 0) == g._lib.ERR_INVALID_ARGUMENT
    assert L.gpf_set_block_params(None, None, 0, 0) == g._lib.ERR_INVALID_ARGUMENT
    # ... and the rows set before are still in force: the next block steps equal the oracle
    for a, b in zip(snapshot(g, st)[:3], before[:3]):
        assert np.array_equal(a, b)
    g.pf_update_blocks(st, (3,), (None,), ys[:, 2], nb); ref.update(ys[:, 2])
    assert same_state(st, ref)
    # model-independent calls keep working
    g.pf_resample(st, "multinomial", check=False)
    g.get_ess(st); g.get_lml_est(st); g.block_stats(st, nb)
    # cleared: today's behaviour (the filter's own parameters) exactly -- a twin that never had rows
    g.set_block_params(st, None)
    twin = g.DeviceParticleFilterState(m, N, seed=13, keep_prev=True)
    twin.restore(st.checkpoint())
    for x in (st, twin):
        g.pf_update(x, (4,), (None,), ys[0, 3]); g.pf_rejuvenate(x, None, (), 1, method="move")
        g.pf_resize(x, 500, "multinomial")
    assert np.array_equal(st.traces, twin.traces) and np.array_equal(st.log_weights, twin.log_weights) and np.array_equal(st.parents, twin.parents)
    for x in (v, shard, hist, twin, st):
        x.close()


def test_checkpoint_then_set_the_rows_again(g, o):
    N, nb, T = 700, 64, 6
    m, sets, assign, ys, st, ref = setup(g, o, "sv1", N, nb, T=T)
    for t in range(1, 3):
        g.pf_update_blocks(st, (t + 1,), (None,), ys[:, t], nb); ref.update(ys[:, t])
        g.pf_resample_blocks(st, nb, "residual", ess_frac=0.5, check=False); ref.resample("residual", ess_frac=0.5)
    blob = st.checkpoint()
    fresh = g.DeviceParticleFilterState(m, N, seed=13, keep_prev=True).restore(blob)
    g.set_block_params(fresh, [sets[k] for k in assign], nb)
    for t in range(3, T):
        for x in (st, fresh):
            g.pf_update_blocks(x, (t + 1,), (None,), ys[:, t], nb)
            g.pf_resample_blocks(x, nb, "residual", ess_frac=0.5, check=False)
            g.pf_rejuvenate_blocks(x, None, (), 1, method="move", only_resampled=True)
        ref.update(ys[:, t]); mask = ref.resample("residual", ess_frac=0.5); ref.rejuvenate(ys[:, t], "move", mask=mask)
        assert same_state(st, ref) and same_state(fresh, ref), t
    assert np.array_equal(g.block_stats(st, nb)[1], g.block_stats(fresh, nb)[1])
    st.close(); fresh.close()


def test_known_answer_theta_grid(g, o):
    """lgssm2 over a 3 x 3 theta grid, 4 replicate blocks per theta, T = 100 steps of data from one grid point: every theta's estimate lies
    near its Kalman log-likelihood and the data-generating theta ranks first (tolerances rehearsed on the oracle, block_params_spec.py)"""
    ms, ys, assign, N = sp.ka_setup(g.models)
    B = assign.size
    st = g.pf_initialize_blocks(ms[0], (1,), np.tile(ys[0], (B, 1)), N, sp.KA_NB, seed=sp.KA_SEED, params=[ms[k] for k in assign])
    for t in range(1, sp.KA_T):
        g.pf_update_blocks(st, (t + 1,), (None,), np.tile(ys[t], (B, 1)), sp.KA_NB, proposals=[g.locally_optimal] * B)
        g.pf_resample_blocks(st, sp.KA_NB, "residual", ess_frac=0.5, check=False)
    lml = g.block_stats(st, sp.KA_NB)[1]
    est, exact = sp.ka_summary(lml, assign, ms, ys, g.models)
    assert np.all(est - exact > -sp.KA_TOL_BELOW) and np.all(est - exact < sp.KA_TOL_ABOVE), np.round(est - exact, 3)
    assert sp.KA_GRID[int(np.argmax(est))] == sp.KA_TRUE
    st.close()
