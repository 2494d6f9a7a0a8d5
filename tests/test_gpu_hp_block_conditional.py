"""The pinned particle's weight on the device against the mpmath model definitions (tests/hp_reference.py Ref.loglik) with the derived per-value
tolerances of tests/hp_checks.py: slot 0 of every block gets log p(y_b | ref[b]) at the initialisation and lw + log p(y_b | ref[b]) at an update --
the bootstrap weight of the GIVEN value, not of the value the model would have drawn.  One step of each kind per model."""
import numpy as np
import pytest

import hp_checks as hc
import hp_reference as hp
from hp_reference import E

pytestmark = pytest.mark.gpu

SEED, NB, N = 20240917, 7, 7 * 9 + 3                                          # nine full blocks and a short one


def pinned_values(g, m, B, ys):
    """[B, 2, d] latent values the model itself could have produced: slot 0 of a plain filter of another seed, at the two steps"""
    st = g.pf_initialize_blocks(m, (1,), np.tile(ys[0], (B, 1)), B * NB, NB, seed=SEED + 1)
    first = st.traces[::NB, :m.dim].copy()
    g.pf_update_blocks(st, (2,), (None,), np.tile(ys[1], (B, 1)), NB)
    second = st.traces[::NB, :m.dim].copy()
    st.close()
    return np.stack([first, second], axis=1)


@pytest.mark.parametrize("keep_prev", [False, True])
@pytest.mark.parametrize("name", ["lgssm2", "bearings4", "sv1", "object_motion"])
def test_pinned_weight_increment(g, name, keep_prev):
    m = g.models.by_name(name)
    ref_model = hp.Ref(m)
    B = (N + NB - 1) // NB
    ys = hc.case_data(g, m, 2)
    obs = ys[:, None, :] + 0.05 * np.random.default_rng(3).standard_normal((2, B, ys.shape[1]))      # every block its own data
    if name == "object_motion":
        obs[..., 1] = ys[:, None, 1]                                          # (the second entry is the model's input sin(t), not a measurement)
    x = pinned_values(g, m, B, ys)
    b0 = np.arange(0, N, NB)
    st = g.pf_initialize_blocks(m, (1,), obs[0], N, NB, seed=SEED, keep_prev=keep_prev, reference=x[:, 0])
    rows, lw0 = st.traces, st.log_weights
    v = hc.Violations()
    for b, i in enumerate(b0):
        for k in range(m.dim):
            v.exact(f"initialize x[{k}]", i, rows[i, k], x[b, 0, k])
        v.value("pinned initialize lw", i, lw0[i], ref_model.loglik(list(x[b, 0]), obs[0, b]))
    v.finish(f"{name} pinned initialize")
    g.pf_update_blocks(st, (2,), (None,), obs[1], NB, reference=x[:, 1])
    rows, lw = st.traces, st.log_weights
    v = hc.Violations()
    for b, i in enumerate(b0):
        for k in range(m.dim):
            v.exact(f"update x[{k}]", i, rows[i, k], x[b, 1, k])
            if keep_prev:
                v.exact(f"update x_prev[{k}]", i, rows[i, m.dim + k], x[b, 0, k])
        v.value("pinned update lw", i, lw[i], E(lw0[i]) + ref_model.loglik(list(x[b, 1]), obs[1, b]))
    v.finish(f"{name} pinned update")
    st.close()
