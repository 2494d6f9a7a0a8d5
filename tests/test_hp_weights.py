"""The CPU oracle's weight side -- fixed-point weights, the integer CDF, the resampling uniforms, ancestors of the three resamplers and of
pf_resize, the weights after a resample, the log-ML bookkeeping, ESS, the normalised weights, mean / var / proportionmap and their block-wise
forms -- against tests/hp_weights.py: the definitions of src/resample.jl, src/resize.jl, src/utils.jl and src/statistics.jl in mpmath on exact
uniforms.  A decision (an ancestor, a copy count, the ESS verdict) is compared wherever it is decidable within the quantisation bound DERIVED
in hp_weights.py; a value within its derived bound.  tests/test_gpu_hp_weights.py runs the same cases on the device.

What the cases catch that "device == oracle" cannot: a slot reading the wrong word pair or stratum, a biased residual tail, the log-ML
increment from the priorities, a flipped sign in the tempered weights, a dropped limb of sum q^2, a variance centred on the wrong mean.

Sizes: the smallest at which each path changes (a wave and one past it; K 52 -> 51 at 1024 / 1025, S = 2^62 exactly at 1024 equal weights;
one scan tile and the start of the chain at 2047 / 2048 / 2049; the third tile at 4097); block sizes at the three team shapes and their edges.

The rest of src/resize.jl the same way: the optimal resize (threshold, keep set, systematic picks, both kinds of weight), pf_dereplicate with
method="sample" and the replicate / keepfirst round trip, pf_coalesce over the key shapes that steer the in-wave merge of the kernels, and
pf_introduce (every new particle's chain under mix(seed, epoch) of include/gpf.h, tests/hp_checks.py Run.introduce).  The tests named
test_rejects_* hand the checker a perturbed result through the oracle adapter: each must be rejected."""
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
    # pf_dereplicate(method="sample"): output j reads words (0,1) of block j -- the word pair of slot 2j, not of slot j
    for j in list(range(70)) + [4096, 2 ** 31 - 1]:
        U = hw.dereplicate_u64(seed, j, 7)
        assert o.lib().o_resample_u52_d(seed, 2 * j, 7) == ((U >> 12) + 0.5) * 2.0 ** -52, j
    assert hw.dereplicate_u64(seed, 5, 7) != hw.resample_u64(seed, 5, 7)


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


# ------------------------------------------------------------------------------------------- pf_resize(..., "optimal") (resize.jl:149-219)
# (n, n', weight vector, the number of kept particles by the reference alone; None: whatever the definition gives)
OPTIMAL = [(2049, 1025, "spread", 376), (2049, 1025, "plus700", 376), (2049, 1025, "some_neginf", 636), (2049, 1025, "equal", 0),
           (2049, 2048, "spread", 2043), (2049, 2048, "ulp_apart", 0), (2049, 2048, "some_neginf", 1366),      # the last: 682 drawn uniformly among 683 -Inf
           (2049, 2049, "spread", 2049),                                                                      # the exact identity
           (2049, 65, "wide", 45), (2049, 65, "dead_tail", 0),
           (2049, 1, "dominant", 0), (2049, 2, "dominant", 1),
           (4097, 2049, "spread", 768),                                                                       # two scan tiles plus one; K = 49
           (65, 64, "spread", None), (3, 2, "spread", None), (2, 1, "spread", None), (1, 1, "spread", 1),
           (2049, 1025, "all_neginf", 0)]
OPTIMAL_INVALID = [(2049, 2048, "some_neginf"), (2049, 1025, "all_neginf")]


def optimal_possible(n, n_new, kind):
    """dead_tail: the flushed half weighs e^-720 > 0 in the reals and 0 in the fixed point.  With n' above the live
    count the definition keeps flushed particles the spec cannot see; at n' = the live count the threshold sits on that boundary exactly.
    wide at 4097 -> 2049: the ~2250 unkept particles lie 29 and more below the maximum, at most ~150 counts each at K = 49 and most of them a
    few; the bound of a pick, (2 D' + 3) / S'_lo, comes to 1.5e-3 .. 8 over the seeds 1 .. 14 against strata of 5e-3: every one of the ~200
    picks is undecidable under every seed (and the threshold under most).  `spread` stands at that size instead."""
    if kind == "wide" and n > 2049:
        return False
    return not (kind == "dead_tail" and n_new >= n - n // 2)


assert all(optimal_possible(n, n_new, kind) for n, n_new, kind, _ in OPTIMAL)


def drive_optimal(r, ys, n, n_new, kind, n_keep=None):
    r.initialize(ys[0], check=False)
    r.update(ys[1], check=False)
    r.a.set_lw(weight_vector(kind, n))
    if kind == "all_neginf":
        r.resize_refused(n_new)                                # check=True raises and leaves n = 2049
        assert len(r.a.lw) == n
    left_out = r.resize_optimal(n_new)
    assert n_keep is None or r.n_keep == n_keep, (r.n_keep, n_keep)
    if kind != "all_neginf":
        r.update(ys[2])                                        # the resized filter goes on: every particle id, the new count in log N
    r.check_summaries(addrs=(0,))
    return left_out


@pytest.mark.parametrize("n,n_new,kind,n_keep", OPTIMAL)
def test_optimal_resize(g, o, n, n_new, kind, n_keep):
    r, ys = make_run(hc.OracleAdapter, g, o, n)
    assert drive_optimal(r, ys, n, n_new, kind, n_keep) == 0


# ------------------------------------------------------------------------------------------- pf_dereplicate(..., method="sample") (resize.jl:281-293)
DEREPLICATE = [(k, n_new, layout, kind) for k, n_new in ((2, 1), (3, 65), (64, 65), (2, 2049)) for layout in ("contiguous", "interleaved")
               for kind in ("spread", "wide", "some_neginf")] + [(3, 65, "contiguous", "first_group_neginf"), (3, 65, "interleaved", "first_group_neginf")]


def replicate_vector(kind, k, n_new, layout):
    if kind != "first_group_neginf":
        return weight_vector(kind, k * n_new)
    lw = weight_vector("spread", k * n_new)
    lw[hw.replicate_groups(k * n_new, k, layout)[0]] = -np.inf
    return lw


def drive_dereplicate(r, ys, k, n_new, layout, kind):
    r.initialize(ys[0], check=False)
    r.update(ys[1], check=False)
    r.a.set_lw(replicate_vector(kind, k, n_new, layout))
    left_out = r.dereplicate_sample(k, layout)
    if kind == "first_group_neginf":
        assert r.a.lw[0] == -np.inf
    r.update(ys[2], check=n_new <= 65 and kind != "first_group_neginf")      # the draw consumed an epoch; ids 0 .. n_new - 1
    r.check_summaries(addrs=(0,))
    return left_out


@pytest.mark.parametrize("k,n_new,layout,kind", DEREPLICATE)
def test_dereplicate_sample(g, o, k, n_new, layout, kind):
    r, ys = make_run(hc.OracleAdapter, g, o, k * n_new)
    assert drive_dereplicate(r, ys, k, n_new, layout, kind) == 0


def drive_replicate_round_trip(r, ys, layout):
    r.initialize(ys[0], check=False)
    r.update(ys[1], check=False)
    r.resample("multinomial", alpha=0.5)                       # a running estimate and weights that are not 0
    r.replicate_round_trip(3, layout)
    r.update(ys[2])                                            # no epoch was consumed


@pytest.mark.parametrize("layout", ["contiguous", "interleaved"])
def test_replicate_round_trip(g, o, layout):
    r, ys = make_run(hc.OracleAdapter, g, o, 65)
    drive_replicate_round_trip(r, ys, layout)


def test_reference_uniform_of_dereplicate_is_the_one_the_oracle_draws_with(o):
    """output j reads words (0,1) of block j (test_reference_uniforms_are_the_stream_of_the_spec holds the word pair to the
    oracle's view of it): the oracle's draw on two-point groups of equal weights, whose CDF splits at 1/2, is the top bit of that word pair"""
    seed = (0x1234 << 32) | 0x9abcdef1
    n_new = 70
    idx, out = np.empty(n_new, np.int64), np.empty(n_new)
    o.lib().o_dereplicate_sample(np.zeros(2 * n_new), n_new, 2 * n_new, 2, 0, seed, 7, idx, out)
    assert [int(i) for i in idx] == [2 * j + (hw.dereplicate_u64(seed, j, 7) >> 63) for j in range(n_new)]


# ------------------------------------------------------------------------------------------- pf_coalesce (resize.jl:309-334)
COAL_SIZES = [1, 2, 64, 65, 257, 2047, 2048, 2049]
NAN_A = np.array([0x7FF8000000000123], np.uint64).view(np.float64)[0]


def coalesce_keys(shape, n):
    """group label per particle, as the Float64 that is written into every key column"""
    i = np.arange(n)
    if shape == "mod8":                    # every wave holds 8 groups of 8 lanes: all rounds of the in-wave merge, the rest to the atomics
        return (i % 8).astype(np.float64)
    if shape == "lane0":                   # lane 0 of every wave unique, lanes 1 .. 63 one group: a single lane is left after the first round
        return np.where(i % 64 == 0, i + 1.0, 0.5)
    if shape == "mod2":
        return (i % 2).astype(np.float64)
    if shape == "one":
        return np.full(n, 3.25)
    if shape == "signed_zero":             # 0.0 and -0.0 are distinct keys
        return np.where(i % 3 == 0, -0.0, 0.0)
    if shape == "nan":                     # one NaN bit pattern is one group
        return np.where(i % 3 == 0, NAN_A, i % 3 + 0.0)
    if shape == "late_max":                # member 0 and member 2048 one group, its maximum in the later tile; every other row its own
        k = i + 1.0; k[0] = k[n - 1] = 0.25
        return k
    if shape == "deep":                    # group 0: members more than 708 below its maximum; group 1: all -Inf; group 2: plain
        return (i % 3).astype(np.float64)
    raise ValueError(shape)


COALESCE = ([("mod8", n) for n in COAL_SIZES] + [("lane0", n) for n in COAL_SIZES if n >= 64] + [("mod2", 2049), ("mod2", 2), ("mod2", 1), ("one", 2049), ("one", 1)]
            + [("signed_zero", 65), ("nan", 65), ("late_max", 2049), ("deep", 257)])


def coalesce_weights(shape, n):
    lw = weight_vector("spread", n)
    if shape == "late_max":
        lw[0], lw[n - 1] = -3.0, 2.5
    if shape == "deep":
        lw[0::3][1::2] -= 715.0
        lw[1::3] = -np.inf
    return lw


def drive_coalesce(r, ys, shape, n):
    r.initialize(ys[0], check=False)
    r.update(ys[1], check=False)
    rows = r.a.rows
    rows[:, :] = coalesce_keys(shape, n)[:, None]
    r.a.set_rows(rows)
    r.a.set_lw(coalesce_weights(shape, n))
    G = r.coalesce()
    assert G == len(set(coalesce_keys(shape, n).view(np.uint64).tolist()))
    if shape != "nan":                                         # (NaN rows have no next step; a weight of -Inf has no bound to check)
        r.update(ys[2], check=shape != "deep")
    assert r.resample("multinomial") <= hc.MAX_UNDECIDABLE
    return G


@pytest.mark.parametrize("shape,n", COALESCE)
def test_coalesce_key_shapes(g, o, shape, n):
    r, ys = make_run(hc.OracleAdapter, g, o, n)
    drive_coalesce(r, ys, shape, n)


def drive_coalesce_natural(r, ys, n):
    """the duplicates a multinomial resample leaves, keyed by every column of a keep_prev row"""
    r.initialize(ys[0], check=False)
    r.update(ys[1], check=False)
    r.resample("multinomial")
    r.update(ys[2], check=False)
    r.resample("multinomial")
    r.a.set_lw(weight_vector("spread", n))
    G = r.coalesce()
    assert 1 < G < n
    r.update(ys[3])
    assert r.resample("multinomial") <= hc.MAX_UNDECIDABLE


def test_coalesce_after_a_resample(g, o):
    r, ys = make_run(hc.OracleAdapter, g, o, 2049)
    drive_coalesce_natural(r, ys, 2049)


def drive_coalesce_by_column(r, ys, n, keep_prev):
    """bearings4 with keep_prev: W = 8, `by` one column, every other column distinct.  sv1 without keep_prev: W = 2 with a padding column
    that is made distinct in every row and is never part of the key."""
    r.a.keep_prev = keep_prev
    r.initialize(ys[0], check=False)
    r.update(ys[1], check=False)
    rows = r.a.rows
    if keep_prev:
        assert rows.shape[1] == 8
        rows[:, 1] = np.arange(n) % 5
        G = 5
    else:
        assert rows.shape[1] == 2 and r.d == 1
        rows[:, 0], rows[:, 1], G = np.arange(n) % 7, np.arange(1.0, n + 1.0), 7
    r.a.set_rows(rows)
    r.a.set_lw(weight_vector("wide", n))
    assert r.coalesce((1,) if keep_prev else None) == G
    if keep_prev:
        r.update(ys[2])
    assert r.resample("multinomial") <= hc.MAX_UNDECIDABLE


@pytest.mark.parametrize("name,keep_prev", [("bearings4", True), ("sv1", False)])
def test_coalesce_by_a_column_and_the_padding(g, o, name, keep_prev):
    r, ys = make_run(hc.OracleAdapter, g, o, 2049, name)
    drive_coalesce_by_column(r, ys, 2049, keep_prev)


# ------------------------------------------------------------------------------------------- pf_introduce (resize.jl:351-421)
# (model, T, proposal, (n_old, n_add)): every model at T = 1, 2, 5, every size with and without a stored x_{T-1} behind a carried chain
INTRODUCE = [("lgssm2", 1, False, (64, 1)), ("lgssm2", 2, False, (65, 257)), ("lgssm2", 5, False, (2049, 255)),
             ("bearings4", 1, False, (65, 257)), ("bearings4", 2, False, (64, 1)), ("bearings4", 5, False, (65, 257)),
             ("sv1", 1, False, (2049, 255)), ("sv1", 2, False, (65, 257)), ("sv1", 5, False, (64, 1)),
             ("object_motion", 1, False, (64, 1)), ("object_motion", 2, False, (2049, 255)), ("object_motion", 5, False, (65, 257)),
             ("line_model", 1, False, (65, 257)), ("line_model", 2, False, (64, 1)), ("line_model", 5, False, (2049, 255)),
             ("lgssm2", 1, True, (65, 257)), ("lgssm2", 3, True, (2049, 255)), ("line_model", 1, True, (64, 1))]


def make_intro_run(adapter, g, o, name, n):
    m = g.models.by_name(name)
    return hc.Run(adapter(g, o, m, n, SEED), m, n, SEED), hc.case_data(g, m, 8)


def drive_introduce(r, ys, T, n_add, proposal=False, after_resample=False, twice=False):
    r.initialize(ys[0], check=False)
    for t in range(1, T):
        r.update(ys[t], check=False)
    if after_resample:                                         # log_ml_est != 0 and weights that are not 0: the old weights take the estimate
        r.resample("multinomial", alpha=0.5)
    n_old = r.n
    r.introduce(ys[:T], n_add, proposal)
    if twice:                                                  # the next epoch: another seed, another stream; the estimate is 0 by now
        first = r.a.rows[n_old:].copy()
        r.introduce(ys[:T], n_add, proposal)
        assert not np.array_equal(first, r.a.rows[n_old + n_add:])
    r.update(ys[T])                                            # the epoch advanced by one; ids 0 .. n - 1
    r.check_summaries(addrs=(0,))


@pytest.mark.parametrize("name,T,proposal,sizes", INTRODUCE)
def test_introduce(g, o, name, T, proposal, sizes):
    r, ys = make_intro_run(hc.OracleAdapter, g, o, name, sizes[0])
    drive_introduce(r, ys, T, sizes[1], proposal)


@pytest.mark.parametrize("after_resample,twice", [(True, False), (False, True)])
def test_introduce_after_a_resample_and_twice(g, o, after_resample, twice):
    r, ys = make_intro_run(hc.OracleAdapter, g, o, "lgssm2", 65)
    drive_introduce(r, ys, 2, 257, after_resample=after_resample, twice=twice)


# ------------------------------------------------------------------------------------------- the checks can fail
class Tampered(hc.OracleAdapter):
    """the oracle adapter, handing the checker a result that `tamper(filter, rows before, lw before, epoch before)` has perturbed"""
    tamper = None

    def _around(self, call):
        f = self.f
        rows0, lw0, e0 = f.rows.copy(), f.lw.copy(), f.epoch
        out = call()
        self.tamper(f, rows0, lw0, e0)
        return out

    def resize(self, n_new, method, alpha=None):
        return self._around(lambda: super(Tampered, self).resize(n_new, method, alpha))

    def dereplicate(self, k, layout, method):
        return self._around(lambda: super(Tampered, self).dereplicate(k, layout, method))

    def coalesce(self, cols):
        return self._around(lambda: super(Tampered, self).coalesce(cols))

    def introduce(self, hist, n_add, proposal=False):
        return self._around(lambda: super(Tampered, self).introduce(hist, n_add, proposal))


def rejected(g, o, n, drive, tamper):
    """the honest run passes; the same run through the tampering adapter is rejected by an assertion of the CHECKER (the tampered state is
    computed inside the adapter: an exception from there would not be an AssertionError of hp_checks -- `done` tells them apart)"""
    r, ys = make_run(hc.OracleAdapter, g, o, n)
    drive(r, ys)
    r, ys = make_run(Tampered, g, o, n)
    done = []
    r.a.tamper = lambda *a: (tamper(*a), done.append(1))
    with pytest.raises(AssertionError):
        drive(r, ys)
    assert done == [1], "the tampering itself failed"


def _optimal_then(n, n_new, kind):
    def drive(r, ys):
        r.initialize(ys[0], check=False)
        r.update(ys[1], check=False)
        r.a.set_lw(weight_vector(kind, n))
        r.resize_optimal(n_new)
    return drive


@pytest.mark.parametrize("shift", [-1, 1])
def test_rejects_a_threshold_one_position_off(g, o, shift):
    """keep set, picks and weights recomputed with the threshold at d -+ 1 of the descending order"""
    def tamper(f, rows0, lw0, e0):
        ref = hw.optimal_resize(lw0, f.n, f.seed, e0, threshold_shift=shift)
        par = np.array(ref.keep + ref.picks.anc, np.int64)
        f.rows, f.lw, f.parents = rows0[par].copy(), np.array([float(w.v) for w in ref.weights]), par + 1
    rejected(g, o, 2049, _optimal_then(2049, 1025, "spread"), tamper)


def test_rejects_S_in_place_of_B(g, o):
    """the resampled weight from the whole sum: logsumexp(lw) - log a + ratio"""
    def tamper(f, rows0, lw0, e0):
        ref = hw.optimal_resize(lw0, f.n, f.seed, e0)
        f.lw[ref.n_keep:] = hc.lse(lw0) - np.log(ref.a) + (np.log(f.n) - np.log(len(lw0)))
    rejected(g, o, 2049, _optimal_then(2049, 1025, "spread"), tamper)


def _dereplicate_then(k, n_new, kind):
    def drive(r, ys):
        r.initialize(ys[0], check=False)
        r.update(ys[1], check=False)
        r.a.set_lw(weight_vector(kind, k * n_new))
        r.dereplicate_sample(k, "contiguous")
    return drive


def test_rejects_dereplicate_without_log_k(g, o):
    def tamper(f, rows0, lw0, e0):
        f.lw = f.lw + np.log(3.0)
    rejected(g, o, 195, _dereplicate_then(3, 65, "spread"), tamper)


def test_rejects_dereplicate_draws_from_the_slot_convention(g, o):
    """output j drawing from block j >> 1, the convention of the resample slots"""
    def tamper(f, rows0, lw0, e0):
        ref, _, _ = hw.dereplicate_sample(lw0, 3, "contiguous", f.seed, e0, block_of=lambda j: j >> 1)
        par = np.array(ref.anc, np.int64)
        f.rows, f.parents = rows0[par].copy(), par + 1
    rejected(g, o, 195, _dereplicate_then(3, 65, "spread"), tamper)


def _coalesce_then(shape, n):
    def drive(r, ys):
        r.initialize(ys[0], check=False)
        r.update(ys[1], check=False)
        rows = r.a.rows
        rows[:, :] = coalesce_keys(shape, n)[:, None]
        r.a.set_rows(rows)
        r.a.set_lw(coalesce_weights(shape, n))
        r.coalesce()
    return drive


def test_rejects_coalesce_ratio_exchanged(g, o):
    """log n_old - log n_new where log n_new - log n_old belongs"""
    def tamper(f, rows0, lw0, e0):
        f.lw = f.lw - 2.0 * (np.log(f.n) - np.log(len(lw0)))
    rejected(g, o, 257, _coalesce_then("mod8", 257), tamper)


def test_rejects_a_group_sum_missing_its_smallest_member(g, o):
    """group 3 of `mod8` at n = 257: 32 weights of a standard normal, the smallest a share of about e^-2 / 32 / e^(1/2) ~ 2.5e-3 of the sum at the
    very least e^-8 / 32 e^4 ~ 2e-7: eight orders above the bound of a weight (1e-15)"""
    def tamper(f, rows0, lw0, e0):
        _, want, groups = hw.coalesce(rows0, lw0, range(4), drop_smallest_of=3)
        f.lw[3] = float(want[3].v)
    rejected(g, o, 257, _coalesce_then("mod8", 257), tamper)


def _introduced_with(o, f, seed2, epoch0, n_old, hist):
    """the new particles' rows and weights from the oracle's own step functions under another seed / first epoch"""
    L, n_add = o.lib(), f.n - n_old
    rows, lw = np.zeros((n_add, f.W)), np.zeros(n_add)
    L.o_init(f.model, f.params, seed2, epoch0, n_old, n_add, f.W, np.ascontiguousarray(hist[0]), rows, lw)
    for e in range(1, len(hist)):
        out = np.empty_like(rows)
        L.o_step(f.model, f.params, seed2, epoch0 + e, n_old, n_add, f.W, int(f.keep_prev), np.ascontiguousarray(hist[e]), rows, out, lw)
        rows = out
    f.rows[n_old:], f.lw[n_old:] = rows, lw


def _introduce_then(T, n_add):
    def drive(r, ys):
        ys = hc.case_data(r.a.g, r.model, 8)
        r.initialize(ys[0], check=False)
        for t in range(1, T):
            r.update(ys[t], check=False)
        r.introduce(ys[:T], n_add)
    return drive


def test_rejects_introduce_with_the_unmixed_seed(g, o):
    ys = hc.case_data(g, g.models.by_name("lgssm2"), 8)
    rejected(g, o, 65, _introduce_then(2, 33), lambda f, rows0, lw0, e0: _introduced_with(o, f, f.seed, 0, len(lw0), ys[:2]))


def test_rejects_introduce_with_epochs_from_one(g, o):
    import coalesce_spec as cs
    ys = hc.case_data(g, g.models.by_name("lgssm2"), 8)
    rejected(g, o, 65, _introduce_then(2, 33), lambda f, rows0, lw0, e0: _introduced_with(o, f, cs.intro_seed(f.seed, e0), 1, len(lw0), ys[:2]))


def test_the_honest_introduce_is_what_the_tampering_helper_computes(g, o):
    """the helper of the two controls above with the promised seed and epochs reproduces the specification: the controls differ from it by
    the seed / the first epoch alone"""
    import coalesce_spec as cs
    r, ys = make_intro_run(hc.OracleAdapter, g, o, "lgssm2", 65)
    _introduce_then(2, 33)(r, ys)
    f = r.a.f
    rows, lw = f.rows.copy(), f.lw.copy()
    _introduced_with(o, f, cs.intro_seed(f.seed, f.epoch - 1), 0, 65, ys[:2])
    assert np.array_equal(rows, f.rows) and np.array_equal(lw, f.lw)


if __name__ == "__main__":
    # the table "largest derived bound per quantity" of DESIGN.md 3.3: run the committed cases, print what hp_checks collected
    import sys
    rc = pytest.main([__file__, "-q", "-p", "no:cacheprovider"])
    for k, t in sorted(hc.MAX_TOL.items()):
        print(f"{k:45s} {t:.2g}")
    sys.exit(rc)
