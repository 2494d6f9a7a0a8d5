"""The CPU oracle's weight side -- fixed-point weights, the integer CDF, the resampling uniforms, ancestors of the three resamplers and of
pf_resize, the weights after a resample, the log-ML bookkeeping, ESS, the normalised weights, mean / var / proportionmap and their block-wise
forms -- against tests/hp_weights.py: the definitions of src/resample.jl, src/resize.jl, src/utils.jl and src/statistics.jl in mpmath on exact
uniforms.  A decision (an ancestor, a copy count, the ESS verdict) is compared wherever it is decidable within the quantisation bound DERIVED
in hp_weights.py; a value within its derived bound.  tests/test_gpu_hp_weights.py runs the same cases on the device.

What the cases catch that "device == oracle" cannot: a slot reading the wrong word pair or stratum, a biased residual tail, the log-ML
increment from the priorities, a flipped sign in the tempered weights, a dropped limb of sum q^2, a variance centred on the wrong mean.

Sizes: the smallest at which each path changes (a wave and one past it; K 52 -> 51 at 1024 / 1025, S = 2^62 exactly at 1024 equal weights;
one scan tile and the start of the chain at 2047 / 2048 / 2049; the third tile at 4097); block sizes at the three team shapes and their edges."""
import numpy as np
import pytest

import hp_checks as hc
import hp_weights as hw
from conftest import soak_grid

SEED = 20241105
SIZES = [1, 2, 3, 64, 65, 1024, 1025, 2047, 2048, 2049, 4097]
KINDS = ["spread", "wide", "dominant", "equal", "ulp_apart", "dead_tail", "some_neginf", "all_neginf", "plus700", "minus700"]
FORMS = ["multinomial", "residual", "stratified", "stratified_sorted"]
ALPHAS = [None, 0.5]


def weight_vector(kind, n, seed=1):
    rng = np.random.default_rng([seed, n])
    z = rng.standard_normal(n)
    if kind == "spread":
        return z
    if kind == "wide":                                       # most q_i small
        return 8.0 * z
    if kind == "dominant":
        lw = np.full(n, -30.0); lw[n // 3] = 0.0
        return lw
    if kind == "equal":
        return np.full(n, -1.25)
    if kind == "ulp_apart":
        return np.where(rng.random(n) < 0.5, -0.75, np.nextafter(-0.75, 0.0))
    if kind == "dead_tail":                                  # half the particles more than 708 below the maximum: nonzero weight, q = 0
        lw = z.copy(); h = n - n // 2
        lw[h:] -= 720.0 + 20.0 * rng.random(n - h)
        return lw
    if kind == "some_neginf":
        lw = z.copy(); lw[1::3] = -np.inf
        return lw
    if kind == "all_neginf":
        return np.full(n, -np.inf)
    if kind == "plus700":
        return z + 700.0
    if kind == "minus700":
        return z - 700.0
    raise ValueError(kind)


def possible(n, kind, form, alpha):
    """combinations that have an answer: the residual copy counts of equal weights are exact integers (N w_i = 1: undecidable by construction);
    all -Inf under a priority gives NaN weights (-Inf - -Inf) in the reference too"""
    if form == "residual" and kind in ("equal", "ulp_apart"):
        return False
    if form == "residual" and n == 1:                        # N w = 1 exactly
        return False
    return not (kind == "all_neginf" and alpha is not None)


def committed(n, kind, form, alpha):
    """one representative per code path; the rest of the product is the soak set"""
    if not possible(n, kind, form, alpha):
        return False
    return ((kind == "spread" and form == "multinomial" and alpha is None)                 # every size
            or (kind == "spread" and n in (65, 2049))                                      # every form, with and without a priority
            or (n == 1025 and form == "multinomial" and alpha is None)                     # every weight vector
            or (n == 2049 and kind in ("wide", "dead_tail", "some_neginf", "all_neginf") and alpha is None)
            or (n == 1024 and kind == "equal" and alpha is None)                           # S = 2^62 exactly
            or (n == 2 and kind == "ulp_apart" and form == "stratified_sorted")
            or (n == 4097 and kind == "wide" and form == "residual" and alpha == 0.5)
            or (n == 3 and kind == "dominant" and form == "residual" and alpha is None))


GRID = [p for p in soak_grid(SIZES, KINDS, FORMS, ALPHAS, keep=committed) if possible(*p.values)]


def make_run(adapter, g, o, n, name="lgssm2", seed=SEED, history=False):
    m = g.models.by_name(name)
    a = adapter(g, o, m, n, seed)
    a.history = history
    return hc.Run(a, m, n, seed), hc.case_data(g, m, 4)


def drive_case(r, ys, n, kind, form, alpha):
    """rows from a real initialize + update; the weight vector set through the state; getters, the resample, getters again"""
    r.initialize(ys[0], check=False)
    r.update(ys[1], check=False)
    r.a.set_lw(weight_vector(kind, n))
    r.check_summaries(addrs=(0,))
    method, sort = ("stratified", form == "stratified_sorted") if form.startswith("stratified") else (form, True)
    left_out = r.resample(method, alpha=alpha, sort_particles=sort)
    r.check_summaries(addrs=(1,))
    return left_out


@pytest.mark.parametrize("n,kind,form,alpha", GRID)
def test_resample(g, o, n, kind, form, alpha):
    r, ys = make_run(hc.OracleAdapter, g, o, n)
    assert drive_case(r, ys, n, kind, form, alpha) == 0        # by the reference alone: no committed case has an undecidable slot


def test_reference_uniforms_are_the_stream_of_the_spec(o):
    """slot s reads counter (s >> 1, 0, epoch, resample tag), words (0,1) for even s and (2,3) for odd s, here against the
    oracle's 52-bit view of the same word pair; the two slots of a block differ"""
    seed = (0x1234 << 32) | 0x9abcdef1
    for slot in list(range(70)) + [4096, 4097, 2 ** 31 + 1]:
        U = hw.resample_u64(seed, slot, 7)
        assert o.lib().o_resample_u52_d(seed, slot, 7) == ((U >> 12) + 0.5) * 2.0 ** -52, slot
    assert hw.resample_u64(seed, 10, 7) != hw.resample_u64(seed, 11, 7)


def drive_run(r, ys):
    """updates and resamples of every form in one run: the log-ML estimate carried through, tempered weights feeding the next update"""
    r.initialize(ys[0], check=False)
    r.update(ys[1], check=False)
    r.resample("multinomial", alpha=0.5)
    r.check_summaries(addrs=(0, 1))
    r.update(ys[2])                                        # checked: the tempered weights are what this update adds to
    r.resample("stratified", alpha=0.5, sort_particles=True)
    r.update(ys[3], check=False)
    r.resample("residual")
    r.check_summaries(addrs=(0,))


@pytest.mark.parametrize("name,n", [("lgssm2", 2049), ("bearings4", 1025)])
def test_log_ml_through_a_run(g, o, name, n):
    r, ys = make_run(hc.OracleAdapter, g, o, n, name)
    drive_run(r, ys)


def drive_history(r, ys):
    """mean / var / proportionmap of a current-step column and of a past-step address behind two resamples"""
    r.initialize(ys[0], check=False)
    r.update(ys[1], check=False)
    r.resample("multinomial")
    r.update(ys[2], check=False)
    r.resample("stratified", alpha=0.5)
    r.update(ys[3], check=False)
    r.check_summaries(addrs=(1, (1, 1), (2, 1)), discrete=(0, (2, 0)))


@pytest.mark.parametrize("n", [65, 2049])
def test_statistics_of_current_and_past_addresses(g, o, n):
    r, ys = make_run(hc.OracleAdapter, g, o, n, "object_motion", history=True)
    drive_history(r, ys)


@pytest.mark.parametrize("n", [64, 1025, 2049])
def test_step_ess_verdict(g, o, n):
    """the verdict ESS < threshold N at thresholds on both sides of the ESS; the resample inside the call is checked like any other"""
    r, ys = make_run(hc.OracleAdapter, g, o, n)
    drive_step_ess(r, ys)


def drive_step_ess(r, ys):
    """ESS lies in [1, N]: 0.999 N is above it after an update, 1e-4 N (< 1 at these sizes) below"""
    r.initialize(ys[0], check=False)
    went = [r.step_ess(ys[t], thr, must_decide=True) for t, thr in ((1, 0.999), (2, 1e-4), (3, 0.5))]
    assert went[0] and not went[1]


BLOCK_SIZES = [100, 128, 129, 512, 513, 2048]


def drive_blocks(r, ys, nb, n_blocks):
    """block b is the sub-state of its particles; one block all -Inf, one wide, the others spread"""
    r.initialize(ys[0], check=False)
    r.update(ys[1], check=False)
    lw = np.concatenate([weight_vector(["spread", "all_neginf", "wide", "dead_tail", "spread"][b], nb, seed=b + 1) for b in range(n_blocks)])
    r.a.set_lw(lw)
    r.check_blocks(nb, col=1, discrete_col=0)


@pytest.mark.parametrize("nb", BLOCK_SIZES)
def test_block_estimates(g, o, nb):
    n_blocks = 3 if nb == 2048 else 4
    r, ys = make_run(hc.OracleAdapter, g, o, nb * n_blocks, "object_motion")
    drive_blocks(r, ys, nb, n_blocks)


RESIZES = [(2048, "multinomial", None), (2050, "multinomial", 0.5), (4099, "multinomial", None), (1, "multinomial", None),
           (2048, "residual", None), (2050, "residual", None), (4099, "residual", 0.5), (1, "residual", None)]


def drive_resize(r, ys, n_new, method, alpha):
    r.initialize(ys[0], check=False)
    r.update(ys[1], check=False)
    left_out = r.resize(n_new, method, alpha=alpha)
    r.update(ys[2], check=n_new <= 2050)                                        # the resized filter goes on: every particle id, the new count in log N
    r.check_summaries(addrs=(0,))
    return left_out


@pytest.mark.parametrize("n_new,method,alpha", RESIZES)
def test_resize(g, o, n_new, method, alpha):
    r, ys = make_run(hc.OracleAdapter, g, o, 2049)
    assert drive_resize(r, ys, n_new, method, alpha) == 0


def test_sample_unweighted(g, o):
    r, ys = make_run(hc.OracleAdapter, g, o, 2049)
    r.initialize(ys[0], check=False)
    r.update(ys[1], check=False)
    assert r.sample_unweighted(65) == 0
    r.update(ys[2])                                        # the draw consumed an epoch


if __name__ == "__main__":
    # the table "largest derived bound per quantity" of DESIGN.md 3.3: run the committed cases, print what hp_checks collected
    import sys
    rc = pytest.main([__file__, "-q", "-p", "no:cacheprovider"])
    for k, t in sorted(hc.MAX_TOL.items()):
        print(f"{k:45s} {t:.2g}")
    sys.exit(rc)
