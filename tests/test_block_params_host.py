"""Per-block model parameters (gpf.h gpf_set_block_params) without a device: the exported symbol and its ctypes entry, the host-side packing and
validation of the rows, the oracle's restricted block loop, and the rehearsal of the known-answer test of tests/test_gpu_block_params.py."""
import ctypes

import numpy as np
import pytest

import block_params_spec as sp


def test_symbol_exported_and_in_the_ctypes_table(g):
    L = ctypes.CDLL(g._lib.LIB_PATH)
    assert hasattr(L, "gpf_set_block_params")
    entry = [s for s in g._lib.SYMBOLS if s[0] == "gpf_set_block_params"]
    assert len(entry) == 1 and entry[0][1] is ctypes.c_int
    assert entry[0][2] == [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.c_int32, ctypes.c_int64]


def test_rows_from_native_models(g):
    m = g.models
    ms = [m.lgssm2(rho=0.9, sr=0.3), m.lgssm2(rho=0.95), m.lgssm2(sr=0.8)]
    rows = g.block_params_rows(m.lgssm2(), ms, 250, 100)                     # 3 blocks: 100, 100, 50 particles
    assert rows.shape == (3, m.lgssm2().params.size) and rows.dtype == np.float64 and rows.flags.c_contiguous
    for k in range(3):
        assert np.array_equal(rows[k], ms[k].params)                          # derived constants come from the constructors, bit for bit
    # block_size is clamped to the particle count: one block
    assert g.block_params_rows(m.sv1(), [m.sv1(phi=0.5)], 10, 1 << 40).shape == (1, 5)
    # the array form passes through unchanged
    arr = np.stack([x.params for x in ms])
    assert np.array_equal(g.block_params_rows(m.lgssm2(), arr, 300, 100), arr)


@pytest.mark.parametrize("case", ["other_model", "row_count", "width", "block_size", "mixture", "ragged"])
def test_bad_rows_raise_before_the_device(g, case):
    m = g.models
    args = {
        "other_model": ([m.lgssm2(), m.sv1()], 200, 100),
        "row_count": ([m.lgssm2()] * 3, 200, 100),
        "width": (np.zeros((2, 5)), 200, 100),
        "block_size": ([m.lgssm2()] * 2, 200, 0),
        "mixture": ([m.lgssm2(), m.lgssm2().params], 200, 100),
        "ragged": ([m.lgssm2(), m.NativeModel(m.MODEL_LGSSM2, "lgssm2", 2, 2, np.zeros(7))], 200, 100),
    }[case]
    with pytest.raises(g.ErrorException):
        g.block_params_rows(m.lgssm2(), *args)


def test_restricted_oracle_loop_equals_the_block_helpers(o, g):
    """ParamBlocksOracle(own_only=True) -- the rehearsal's shortcut -- composes the same state as the repository's block helpers run over all blocks"""
    m = g.models
    ps = [m.lgssm2(rho=0.9).params, m.lgssm2(sr=0.8).params, m.lgssm2(theta=0.3).params]
    N, nb = 730, 64
    B = (N + nb - 1) // nb
    assign = (np.arange(B) * 7 + 1) % 3
    ys = np.asarray(m.simulate(m.lgssm2(), 5))
    obs = ys[None, :, :] + 0.2 * np.random.default_rng(3).standard_normal((B,) + ys.shape)
    refs = [sp.ParamBlocksOracle(o, m.MODEL_LGSSM2, ps, assign, N, nb, 5, keep_prev=True, own_only=own) for own in (False, True)]
    for r in refs:
        r.initialize(obs[:, 0])
    for t in range(1, 5):
        masks = []
        for r in refs:
            r.update(obs[:, t], proposals=(np.arange(B) + t) % 2 == 0)
            masks.append(r.resample("residual", ess_frac=0.7))
        assert np.array_equal(masks[0], masks[1])
        accs = [r.rejuvenate(obs[:, t], "move", mask=masks[0]) for r in refs]
        assert accs[0] == accs[1]
        for attr in ("rows", "lw", "parents"):
            assert np.array_equal(getattr(refs[0], attr), getattr(refs[1], attr)), (attr, t)
    assert np.array_equal(refs[0].block_lml(), refs[1].block_lml())


def test_known_answer_rehearsal_on_the_oracle(o, g):
    """the theta-grid check of tests/test_gpu_block_params.py on the oracle: every theta's estimate near its Kalman log-likelihood, the
    data-generating theta first.  The device reproduces these numbers bit for bit, so the tolerances and seeds are fixed here."""
    lml, assign, ms, ys = sp.ka_oracle(o, g.models)
    est, exact = sp.ka_summary(lml, assign, ms, ys, g.models)
    assert np.all(est - exact > -sp.KA_TOL_BELOW) and np.all(est - exact < sp.KA_TOL_ABOVE), np.round(est - exact, 3)
    assert sp.KA_GRID[int(np.argmax(est))] == sp.KA_TRUE
    assert sp.KA_GRID[int(np.argmax(exact))] == sp.KA_TRUE
