"""Launch census of the cached weight summaries ("The weight-summary cache").  What the handle remembers about the current
log-weights -- the producer's maximum, a scan's CDF, a reduction's sums -- decides which kernels a call launches, and launches are the only
outside sign of it: a flag dropped too late returns a stale value (the oracle comparisons catch that), one dropped too early or never set
costs an extra k_max_partial or scan (only this file catches that).  Every script below asserts, call by call, the launch counts of the six
kernel ids of gpf_kernel_time (STEP, MAX, SCAN, SEARCH, GATHER, MOVE) against a literal table, and the values against the oracle where it
has them.  The table was recorded on the build in front of the change that gathered the flags into WeightSummary (profiles/
weight_summary_state.md says which commit and run) and holds for every later one: a row that changes is a change of the state machine.

Sizes: 7 (one tile, one workgroup) and 70 001 (several tiles, several workgroups of k_sum_host).  `python tests/test_gpu_summary_state.py
SCRIPT N` prints the observed rows of one script as JSON (the child processes of the A/B test, and how the table was recorded)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (7, 70_001)


class Census:
    """launch counts per kernel id of one or more handles; row(label) = the counts since the last row / skip, handle after handle"""

    def __init__(self, *states):
        self.states, self.rows = states, []
        for st in states:
            for k in range(6):
                st.kernel_timing(k, True)
        self.last = self._now()

    def _now(self):
        return [st.kernel_time(k)[1] for st in self.states for k in range(6)]

    def row(self, label):
        now = self._now()
        self.rows.append([label] + [a - b for a, b in zip(now, self.last)])
        self.last = now

    def skip(self):
        """forget what the value comparisons launched (row reads, parents): they are not part of the census"""
        self.last = self._now()


def _pair(g, o, N, seed=2, name="lgssm2"):
    model = g.models.by_name(name); ys = g.models.simulate(model, 9)
    st = g.pf_initialize(model, (1,), ys[0], N, seed=seed, keep_prev=True)
    orc = o.OracleFilter(model.model_id, model.params, N, seed, keep_prev=True).initialize(ys[0])
    return st, orc, ys


def _ess(g, c, st, orc, label):
    e = g.get_ess(st); c.row(label)
    if orc is not None:
        assert e == orc.effective_sample_size(), label
    return e


def _lml(g, c, st, orc, label):
    l = g.get_lml_est(st); c.row(label)
    if orc is not None:
        assert l == orc.log_ml_estimate(), label
    return l


def _same_state(c, st, orc):
    assert np.array_equal(st.log_weights, orc.lw) and np.array_equal(st.traces, orc.rows)
    c.skip()


def script_getters(g, o, N):
    st, orc, ys = _pair(g, o, N); c = Census(st)
    _ess(g, c, st, orc, "ess"); _lml(g, c, st, orc, "lml"); _ess(g, c, st, orc, "ess again")
    g.pf_update(st, (2,), (None,), ys[1]); orc.update(ys[1]); c.row("update")
    _lml(g, c, st, orc, "lml after update"); _ess(g, c, st, orc, "ess after update")
    return c.rows


def script_residual_after_read(g, o, N):
    st, orc, ys = _pair(g, o, N); c = Census(st)
    _ess(g, c, st, orc, "ess")
    g.pf_resample(st, "residual", check=False); orc.resample("residual", check=False); c.row("resample residual")
    g.pf_update(st, (2,), (None,), ys[1]); orc.update(ys[1]); c.row("update")
    assert np.array_equal(st.parents, orc.parents)
    _same_state(c, st, orc)
    _ess(g, c, st, orc, "ess after update")
    return c.rows


def script_scan_reuse(g, o, N):
    st, orc, ys = _pair(g, o, N); c = Census(st)
    lnw = g.get_log_norm_weights(st); c.row("log_norm_weights")
    # (lw - logsumexp(lw): the two sides may round the logarithm of the exact sum differently, a few ulp of |lw| + |lse| < 10^3)
    np.testing.assert_allclose(lnw, orc.log_norm_weights(), rtol=0, atol=1e-12)
    _ess(g, c, st, orc, "ess")
    g.pf_resample(st, "multinomial", check=False); orc.resample("multinomial", check=False); c.row("resample multinomial")
    g.pf_update(st, (2,), (None,), ys[1]); orc.update(ys[1]); c.row("update")
    assert np.array_equal(st.parents, orc.parents)
    _same_state(c, st, orc)
    _lml(g, c, st, orc, "lml after update")
    return c.rows


def script_written_weights(g, o, N):
    st, orc, ys = _pair(g, o, N); c = Census(st)
    _ess(g, c, st, orc, "ess")
    lw = -3.0 * np.random.default_rng(N).random(N)
    st.log_weights = lw; orc.lw = lw.copy(); c.row("set log_weights")
    _ess(g, c, st, orc, "ess (MAX runs)"); _ess(g, c, st, orc, "ess again"); _lml(g, c, st, orc, "lml")
    return c.rows


def script_reweight_move(g, o, N):
    st, orc, ys = _pair(g, o, N); c = Census(st)
    g.pf_update(st, (2,), (None,), ys[1]); orc.update(ys[1]); c.row("update")
    _ess(g, c, st, orc, "ess")
    g.pf_rejuvenate(st, None, (), 1, method="reweight", count=True); orc.rejuvenate("reweight", 1); c.row("rejuvenate reweight, counted")
    assert st.n_accepted == N
    _ess(g, c, st, orc, "ess (no MAX)"); _lml(g, c, st, orc, "lml")
    g.pf_resample(st, "multinomial", check=False); orc.resample("multinomial", check=False); c.row("resample multinomial")
    g.pf_rejuvenate(st, None, (), 1, method="move", count=True); orc.rejuvenate("move", 1); c.row("rejuvenate move, counted (fused gather)")
    _ess(g, c, st, orc, "ess after move"); _lml(g, c, st, orc, "lml after move")
    g.pf_rejuvenate(st, None, (), 1, method="move", count=True); orc.rejuvenate("move", 1); c.row("rejuvenate move, counted (no gather)")
    _ess(g, c, st, orc, "ess again (weights untouched)")
    _same_state(c, st, orc)
    return c.rows


def _script_views(g, o, N, start, stop, step):
    st, orc, ys = _pair(g, o, N)
    sub = st[start:stop:step]
    osub = o.OracleSubState(orc, start, sub.n_particles, step)
    c = Census(st, sub)
    _ess(g, c, sub, osub, "ess of sub")
    _ess(g, c, sub, osub, "ess of sub again")
    g.pf_update(st, (2,), (None,), ys[1]); orc.update(ys[1]); c.row("update of st")
    _ess(g, c, sub, osub, "ess of sub (launches again)")
    _ess(g, c, st, orc, "ess of st")
    g.pf_resample(sub, "multinomial", check=False); osub.resample("multinomial", check=False); c.row("resample sub")
    _ess(g, c, st, orc, "ess of st (launches again)")
    _lml(g, c, st, orc, "lml of st")
    _ess(g, c, sub, osub, "ess of sub after its resample")
    _same_state(c, st, orc)
    return c.rows


def script_views(g, o, N):
    return _script_views(g, o, N, 1, N - 2, 1)


def script_views_strided(g, o, N):
    return _script_views(g, o, N, 1, N - 1, 3)


def script_other_writers(g, o, N):
    st, orc, ys = _pair(g, o, N); c = Census(st)

    def both(tag, ost=orc):
        _ess(g, c, st, ost, "ess after " + tag); _lml(g, c, st, ost, "lml after " + tag)

    both("initialize")
    g.pf_resample(st[0:N], "residual", check=False); o.OracleSubState(orc, 0, N).resample("residual", check=False); c.row("resample_local")
    both("resample_local")
    g.pf_update(st, (2,), (None,), ys[1]); orc.update(ys[1]); c.row("update")
    r = g.pf_step_ess(st, (3,), (None,), ys[2], ess_threshold=0.0, method="residual", check=False); c.row("step_ess, no resample")
    orc.update(ys[2])
    assert r is False
    both("step_ess, no resample")
    r = g.pf_step_ess(st, (4,), (None,), ys[3], ess_threshold=1.1, method="residual", check=False); c.row("step_ess, resample")
    orc.resample("residual", check=False); orc.update(ys[3])
    assert r is True
    both("step_ess, resample")
    blob = st.checkpoint(); c.row("checkpoint save")
    both("checkpoint save")
    st.restore(blob); c.row("checkpoint load")
    both("checkpoint load")
    _same_state(c, st, orc)
    # (from here on the values are compared where other tests pin them: test_gpu_blocks.py, test_coalesce.py)
    g.pf_resample_blocks(st, 3 if N < 100 else 1000, "multinomial", check=False); c.row("resample_blocks")
    both("resample_blocks", None)
    M = N - N // 3
    g.pf_resize(st, M, "multinomial", check=False); c.row("resize")
    both("resize", None)
    g.pf_update(st, (5,), (None,), ys[4]); c.row("update after resize")
    g.pf_resample(st, "multinomial", check=False); c.row("resample multinomial")
    g.pf_coalesce(st); c.row("coalesce")
    both("coalesce", None)
    return c.rows


SCRIPTS = {f.__name__[len("script_"):]: f for f in (script_getters, script_residual_after_read, script_scan_reuse, script_written_weights,
                                                    script_reweight_move, script_views, script_views_strided, script_other_writers)}
AB_SCRIPTS = ("getters", "residual_after_read", "scan_reuse")
AB_ENVS = {"scan": {"GPF_SUM_REDUCE": "0"}, "scan+publish kernel": {"GPF_SUM_REDUCE": "0", "GPF_ESS_PUBLISH": "kernel"}}

# (script, variant) -> the counts of every row, in the order STEP MAX SCAN SEARCH GATHER MOVE (views: the filter's six, then the sub-state's).
# One table for both sizes: the recorded rows were the same at 7 and at 70 001 particles.
_VIEW_ROWS = [
    [0, 0, 0, 0, 0, 0, 0, 1, 1, 0, 0, 0],               # ess of sub
    [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],               # ess of sub again
    [1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],               # update of st
    [0, 0, 0, 0, 0, 0, 0, 1, 1, 0, 0, 0],               # ess of sub (launches again)
    [0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0],               # ess of st
    [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 0],               # resample sub
    [0, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0],               # ess of st (launches again)
    [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],               # lml of st
    [0, 0, 0, 0, 0, 0, 0, 1, 1, 0, 0, 0],               # ess of sub after its resample
]
_RESIDUAL_ROWS = [
    [0, 0, 1, 0, 0, 0],                                 # ess
    [0, 0, 1, 1, 0, 0],                                 # resample residual (the residual scan alone: no MAX, no weight scan)
    [1, 0, 0, 0, 0, 0],                                 # update
    [0, 0, 1, 0, 0, 0],                                 # ess after update
]
_SCAN_REUSE_ROWS = [
    [0, 0, 1, 0, 0, 0],                                 # log_norm_weights
    [0, 0, 1, 0, 0, 0],                                 # ess (the scan again, now with sum q^2)
    [0, 0, 0, 1, 0, 0],                                 # resample multinomial (reuses that CDF)
    [1, 0, 0, 0, 0, 0],                                 # update
    [0, 0, 1, 0, 0, 0],                                 # lml after update
]
_SCAN_GETTER_ROWS = [
    [0, 0, 1, 0, 0, 0],                                 # ess
    [0, 0, 0, 0, 0, 0],                                 # lml
    [0, 0, 0, 0, 0, 0],                                 # ess again
    [1, 0, 0, 0, 0, 0],                                 # update
    [0, 0, 1, 0, 0, 0],                                 # lml after update (a scan without sum q^2)
    [0, 0, 1, 0, 0, 0],                                 # ess after update (... so the scan again)
]
EXPECTED = {
    ("getters", "default"): [
        [0, 0, 1, 0, 0, 0],                                 # ess
        [0, 0, 0, 0, 0, 0],                                 # lml
        [0, 0, 0, 0, 0, 0],                                 # ess again
        [1, 0, 0, 0, 0, 0],                                 # update
        [0, 0, 1, 0, 0, 0],                                 # lml after update
        [0, 0, 0, 0, 0, 0],                                 # ess after update
    ],
    ("residual_after_read", "default"): _RESIDUAL_ROWS,
    ("scan_reuse", "default"): _SCAN_REUSE_ROWS,
    ("written_weights", "default"): [
        [0, 0, 1, 0, 0, 0],                                 # ess
        [0, 0, 0, 0, 0, 0],                                 # set log_weights
        [0, 1, 1, 0, 0, 0],                                 # ess (MAX runs)
        [0, 0, 0, 0, 0, 0],                                 # ess again
        [0, 0, 0, 0, 0, 0],                                 # lml
    ],
    ("reweight_move", "default"): [
        [1, 0, 0, 0, 0, 0],                                 # update
        [0, 0, 1, 0, 0, 0],                                 # ess
        [0, 0, 0, 0, 0, 1],                                 # rejuvenate reweight, counted
        [0, 0, 1, 0, 0, 0],                                 # ess (no MAX)
        [0, 0, 0, 0, 0, 0],                                 # lml
        [0, 0, 1, 1, 0, 0],                                 # resample multinomial
        [0, 0, 0, 0, 0, 1],                                 # rejuvenate move, counted (fused gather)
        [0, 1, 1, 0, 0, 0],                                 # ess after move
        [0, 0, 0, 0, 0, 0],                                 # lml after move
        [0, 0, 0, 0, 0, 1],                                 # rejuvenate move, counted (no gather)
        [0, 0, 0, 0, 0, 0],                                 # ess again (weights untouched)
    ],
    ("views", "default"): _VIEW_ROWS,
    ("views_strided", "default"): _VIEW_ROWS,
    ("other_writers", "default"): [
        [0, 0, 1, 0, 0, 0],                                 # ess after initialize
        [0, 0, 0, 0, 0, 0],                                 # lml after initialize
        [0, 0, 2, 1, 0, 0],                                 # resample_local
        [0, 1, 1, 0, 1, 0],                                 # ess after resample_local
        [0, 0, 0, 0, 0, 0],                                 # lml after resample_local
        [1, 0, 0, 0, 0, 0],                                 # update
        [1, 0, 1, 0, 0, 0],                                 # step_ess, no resample
        [0, 0, 1, 0, 0, 0],                                 # ess after step_ess, no resample
        [0, 0, 0, 0, 0, 0],                                 # lml after step_ess, no resample
        [1, 0, 1, 1, 0, 0],                                 # step_ess, resample
        [0, 0, 1, 0, 0, 0],                                 # ess after step_ess, resample
        [0, 0, 0, 0, 0, 0],                                 # lml after step_ess, resample
        [0, 0, 0, 0, 0, 0],                                 # checkpoint save
        [0, 0, 0, 0, 0, 0],                                 # ess after checkpoint save
        [0, 0, 0, 0, 0, 0],                                 # lml after checkpoint save
        [0, 0, 0, 0, 0, 0],                                 # checkpoint load
        [0, 1, 1, 0, 0, 0],                                 # ess after checkpoint load
        [0, 0, 0, 0, 0, 0],                                 # lml after checkpoint load
        [0, 0, 0, 1, 0, 0],                                 # resample_blocks
        [0, 1, 1, 0, 0, 0],                                 # ess after resample_blocks
        [0, 0, 0, 0, 0, 0],                                 # lml after resample_blocks
        [0, 0, 1, 0, 0, 0],                                 # resize
        [0, 1, 1, 0, 0, 0],                                 # ess after resize
        [0, 0, 0, 0, 0, 0],                                 # lml after resize
        [1, 0, 0, 0, 0, 0],                                 # update after resize
        [0, 0, 1, 1, 0, 0],                                 # resample multinomial
        [0, 0, 0, 0, 1, 0],                                 # coalesce
        [0, 1, 1, 0, 0, 0],                                 # ess after coalesce
        [0, 0, 0, 0, 0, 0],                                 # lml after coalesce
    ],
    ("getters", "scan"): _SCAN_GETTER_ROWS,
    ("residual_after_read", "scan"): _RESIDUAL_ROWS,
    ("scan_reuse", "scan"): _SCAN_REUSE_ROWS,
    ("getters", "scan+publish kernel"): _SCAN_GETTER_ROWS,
    ("residual_after_read", "scan+publish kernel"): _RESIDUAL_ROWS,
    ("scan_reuse", "scan+publish kernel"): _SCAN_REUSE_ROWS,
}


def _check(key, rows):
    got = [r[1:] for r in rows]
    print(f"\n    {key!r}: {json.dumps(got)},")
    for r in rows:
        print(f"        # {r[0]}: {r[1:]}")
    want = EXPECTED[(key[0], key[2])]
    assert len(got) == len(want), key
    for r, w in zip(rows, want):
        assert r[1:] == w, (key, r[0], r[1:], w)


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("script", sorted(SCRIPTS))
def test_launch_census(g, o, script, N):
    _check((script, N, "default"), SCRIPTS[script](g, o, N))


@pytest.mark.parametrize("script", AB_SCRIPTS)
@pytest.mark.parametrize("variant", sorted(AB_ENVS))
def test_launch_census_of_the_scan_backed_getters(variant, script):
    """GPF_SUM_REDUCE=0: the getters take the scan (raw_has_q, raw_q_folded); with GPF_ESS_PUBLISH=kernel the separate publish launch folds
    sum q^2.  The switches are read once per process: every run is a fresh child"""
    env = dict(os.environ); env.update(AB_ENVS[variant])
    p = subprocess.run([sys.executable, os.path.abspath(__file__), script, str(SIZES[1])], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    _check((script, SIZES[1], variant), json.loads(p.stdout.strip().splitlines()[-1]))


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    import gpf_amd
    from oracle import oracle
    oracle.lib()
    print(json.dumps(SCRIPTS[sys.argv[1]](gpf_amd, oracle, int(sys.argv[2]))))
