"""The sorted multinomial resampler (GPF_RESAMPLE_MULTINOMIAL_SORTED) on the CPU oracle against tests/hp_weights.py's
sorted_multinomial: the construction in the reals -- spacings -log((k + 1/2) 2^-52) of the slots' uniforms, one Marsaglia-Tsang tile total per
2048 slots, slot j at V_t + (V_{t+1} - V_t) p_j / s_t -- in mpmath, Philox in Python integers, nothing of oracle/ or the library called.  Every
ancestor is compared wherever it is decidable within the slot's own bound, DERIVED in hp_weights.py's docstring; every acceptance decision of
a tile total is asserted decidable by the reference.  tests/test_gpu_hp_sorted_multinomial.py runs the same drivers on the device.

This resampler is the project's own construction: the oracle and the kernels restate it from each other, so an error they share -- the block
of a second attempt, the word pair of a uniform, a shape without its + 1, a tile's RNG id -- is invisible to device == oracle and far below
what the Monte-Carlo checks resolve.  The tests named test_rejects_* hand the checker the ancestors of a perturbed construction (hp_weights
MUTATIONS) next to the correct weights: each must move a decidable slot and be rejected.

Sizes: one slot (shape 2); a wave and one past it; 2047 / 2048 / 2049 (one full tile, shape 2049; a last tile of one slot; the weight scan's
tile); 4096 / 4097 (a full tile between two boundaries; the third tile); 1024 * 2048 + 1 slots (1025 tiles: past the direct placement of the
tiles, Eg = 39) on sampled tiles.  Shape 1 of a tile total is reachable through test_tile_totals alone."""
import functools

import numpy as np
import pytest

import hp_checks as hc
import hp_weights as hw
from conftest import soak_grid
from hp_reference import M, mpf
from test_hp_weights import KINDS, SEED, make_run, weight_vector

SORTED = "multinomial_sorted"
SIZES = [1, 2, 3, 64, 65, 2047, 2048, 2049, 4096, 4097]
ALPHAS = [None, 0.5]

# Seeds found with the reference alone (hp_weights.gamma_tile, no oracle, no device), SEED + k for k = 0, 1, ... at the epoch the drivers
# resample under (2: initialize, update, resample), first hit taken:
#   REJECT_SMALL  the only tile of 3 slots (id 0, shape 4) rejects attempt 0 (k = 212; about 2 % of such tiles do; the tiles of 1 and 2
#                 slots under this seed reject it too)
#   REJECT_LAST   the last tile of 2049 slots (id 2048, shape 2) rejects attempt 0, would accept it on the uniform of words (2,3), and draws another
#                 total from the blocks 2 / 3 than from 3 / 4 (k = 116; the first seed with all three: both attempt controls stand on it)
#   NEGATIVE_V1   the only tile of 1 slot (id 0, shape 2) has 1 + c x <= 0 in attempt 0 (k = 15062; a Float64 pre-filter over 250 000 seeds,
#                 1.5 s, found 14, each confirmed by the reference with the sign decidable)
REJECT_SMALL = (3, SEED + 212)
REJECT_LAST = (2049, SEED + 116)
NEGATIVE_V1 = (1, SEED + 15062)
RESAMPLE_EPOCH = 2


def possible(n, kind, alpha):
    """all -Inf under a priority gives NaN weights (-Inf - -Inf) in the reference too"""
    return not (kind == "all_neginf" and alpha is not None)


def committed(n, kind, alpha):
    if not possible(n, kind, alpha):
        return False
    return ((kind == "spread" and alpha is None)                                           # every size
            or (n == 2049 and alpha is None)                                               # every weight vector
            or (kind == "spread" and n in (65, 4097) and alpha == 0.5)
            or (kind == "equal" and n == 4096 and alpha is None))


GRID = [p for p in soak_grid(SIZES, KINDS, ALPHAS, keep=committed) if possible(*p.values)]


def drive_case(r, ys, n, kind, alpha):
    """rows from a real initialize + update; the weight vector set through the state; the sorted resample; the getters after it"""
    r.initialize(ys[0], check=False)
    r.update(ys[1], check=False)
    assert r.epoch == RESAMPLE_EPOCH
    r.a.set_lw(weight_vector(kind, n))
    left_out = r.resample(SORTED, alpha=alpha)
    r.check_summaries(addrs=(1,))
    return left_out


@pytest.mark.parametrize("n,kind,alpha", GRID)
def test_resample(g, o, n, kind, alpha):
    r, ys = make_run(hc.OracleAdapter, g, o, n)
    assert drive_case(r, ys, n, kind, alpha) == 0              # by the reference alone: no committed case has an undecidable slot


# ------------------------------------------------------------------------------------------- a rejected first attempt
def attempts_of(n, seed, slot0=0):
    """(accepted attempt, attempts with 1 + c x <= 0) per tile of a resample of n slots under RESAMPLE_EPOCH, by the reference"""
    ntl = (n + hw.SP_TILE - 1) // hw.SP_TILE
    out = []
    for t in range(ntl):
        first = t * hw.SP_TILE
        gt = hw.gamma_tile(seed, slot0 + first, RESAMPLE_EPOCH, min(hw.SP_TILE, n - first) + (t == ntl - 1))
        out.append((gt.attempt, gt.negative))
    return out


REJECTED = [REJECT_SMALL, REJECT_LAST, NEGATIVE_V1]


def drive_rejected(r, ys, n, seed):
    """the reference really takes a later attempt in the tile the case was searched for (the last one)"""
    attempt, negative = attempts_of(n, seed)[-1]
    assert attempt >= 1 and negative == ((n, seed) == NEGATIVE_V1), (attempt, negative)
    return drive_case(r, ys, n, "spread", None)


@pytest.mark.parametrize("n,seed", REJECTED)
def test_rejected_first_attempt(g, o, n, seed):
    r, ys = make_run(hc.OracleAdapter, g, o, n, seed=seed)
    assert drive_rejected(r, ys, n, seed) == 0


# ------------------------------------------------------------------------------------------- tile totals alone
TILE_IDS = list(range(300)) + [2048, 4096, 2 ** 31 + 2048, 2 ** 32 - 1]
TILE_NTL = [1, 4, 5, 1024, 1025]                           # Eg = 48, 48, 47, 40, 39


@functools.lru_cache(maxsize=None)
def tile_references(shape):
    return [hw.gamma_tile(9, gid, 3, shape) for gid in TILE_IDS]


def check_tile_totals(shape, total_of):
    """total_of(gid, Eg) -> the integer G = trunc(fl(d v) 2^Eg) under test: within the E bound of d v, plus one count for the truncation"""
    refs = tile_references(shape)
    if shape <= 3:
        assert sum(gt.attempt >= 1 for gt in refs) >= 1        # the later attempts are part of what is compared
    for ntl in TILE_NTL:
        Eg = hw.gamma_E(ntl)
        for gid, gt in zip(TILE_IDS, refs):
            G = int(total_of(gid, Eg))
            off = abs(float(mpf(G) - M.ldexp(gt.value.v, Eg)))
            assert off <= gt.value.e * 2.0 ** Eg + 1.0, (shape, gid, Eg, G, gt.value, gt.attempt)
            assert mpf(G) <= M.ldexp(gt.value.v, Eg) + gt.value.e * 2.0 ** Eg            # a truncation: never above
    hw._worst("gamma_t: |fl(d v) - gamma| / gamma", max(gt.value.e / float(gt.value.v) for gt in refs))


@pytest.mark.parametrize("shape", [1, 2, 3, 17, 2048, 2049])
def test_tile_totals(g, o, shape):
    """o_gamma_tile_d and the host build of the kernels' gamma_tile against the reference's gamma 2^Eg"""
    check_tile_totals(shape, lambda gid, Eg: o.lib().o_gamma_tile_d(9, gid, 3, shape, Eg))
    L = g._lib.load()
    check_tile_totals(shape, lambda gid, Eg: L.gpf_host_gamma_tile(9, gid, 3, shape, Eg))


def test_tile_scale():
    """Eg as the bound reads it: the tile totals' sum fits 62 bits (a total is below 2^12)"""
    assert [hw.gamma_E(ntl) for ntl in TILE_NTL] == [48, 48, 47, 40, 39]
    assert all(ntl * 2 ** 12 * 2 ** hw.gamma_E(ntl) <= 2 ** 62 for ntl in TILE_NTL + [2, 3, 513, 2 ** 20])


# ------------------------------------------------------------------------------------------- a run
def drive_run(r, ys):
    """the README loop's order: the log-ML estimate carried through; tempered weights feed the next update; the first resample's totals
    are drawn by a scan of the call, the second's after a getter left the CDF behind (a launch of their own on the device)"""
    r.initialize(ys[0], check=False)
    r.update(ys[1], check=False)
    r.resample(SORTED, alpha=0.5)
    r.update(ys[2])                                        # checked: the tempered weights are what this update adds to
    r.check_summaries()                                    # effective_sample_size among them
    r.resample(SORTED)
    r.update(ys[3], check=False)
    r.check_summaries(addrs=(0,))


@pytest.mark.parametrize("name,n", [("lgssm2", 2049), ("bearings4", 1025)])
def test_log_ml_through_a_run(g, o, name, n):
    r, ys = make_run(hc.OracleAdapter, g, o, n, name)
    drive_run(r, ys)


def drive_step_ess(r, ys):
    """ESS lies in [1, N]: 0.999 N is above it after an update, 1e-4 N (< 1 at these sizes) below"""
    r.initialize(ys[0], check=False)
    went = [r.step_ess(ys[t], thr, must_decide=True, method=SORTED) for t, thr in ((1, 0.999), (2, 1e-4), (3, 0.999))]
    assert went == [True, False, True]


@pytest.mark.parametrize("n", [64, 2049])
def test_step_ess(g, o, n):
    r, ys = make_run(hc.OracleAdapter, g, o, n)
    drive_step_ess(r, ys)


# ------------------------------------------------------------------------------------------- views
VIEW_N = 4100
VIEWS = [slice(0, 2049, 1), slice(5, 2054, 1), slice(2051, 4100, 1), slice(3, 4100, 7), slice(0, VIEW_N, 1)]
VIEW_CASES = [(sl, SORTED) for sl in VIEWS] + [(sl, m) for sl in VIEWS[:3] for m in ("multinomial", "stratified")]


def drive_view(r, ys, sl, method):
    """[5:2054]: an odd first id flips the word pair of every slot, and both tiles lie off the parent's tile grid"""
    r.initialize(ys[0], check=False)
    r.update(ys[1], check=False)
    return r.resample_view(sl, method)


@pytest.mark.parametrize("sl,method", VIEW_CASES, ids=lambda v: v if isinstance(v, str) else f"{v.start}:{v.stop}:{v.step}")
def test_views(g, o, sl, method):
    r, ys = make_run(hc.OracleAdapter, g, o, VIEW_N)
    assert drive_view(r, ys, sl, method) == 0


def test_view_under_a_priority(g, o):
    r, ys = make_run(hc.OracleAdapter, g, o, VIEW_N)
    r.initialize(ys[0], check=False)
    r.update(ys[1], check=False)
    assert r.resample_view(VIEWS[1], SORTED, alpha=0.5) == 0
    r.update(ys[2])                                        # the view's call consumed an epoch of the parent


# ------------------------------------------------------------------------------------------- many tiles, sampled
MANY_N = 1024 * 2048 + 1                                   # 1025 tiles: the tiles are placed by their own kernel on the device; Eg = 39
MANY_TILES = (0, 1, 511, 1023, 1024)
MANY_EPOCH = 1                                             # a device filter's first resample, straight after initialize


@functools.lru_cache(maxsize=None)
def many_tiles_reference():
    """equal weights: the CDF is i / n exactly and S = n 2^40 (K = 40) whatever the count of one particle is -- no weight-side bound.  All 1025
    totals, the spacings of the sampled tiles only.  {slot: ancestor or None where the slot is undecidable}"""
    n = MANY_N
    st = hw.sorted_targets(SEED, MANY_EPOCH, n, 0, float(n) * 2.0 ** 40, tiles=MANY_TILES)
    want = {}
    for j, x in st.x.items():
        y, e = x * n, st.eps[j] * n
        a = min(int(M.floor(y)), n - 1)
        near = (a > 0 and float(y - a) <= e) or (a < n - 1 and float(a + 1 - y) <= e)
        want[j] = None if near else a
        hw._worst("eps_j: the slot's whole bound", st.eps[j])
    assert sum(a is None for a in want.values()) <= hc.MAX_UNDECIDABLE
    assert len(want) == 4 * hw.SP_TILE + 1
    return want


def check_many_tiles(anc0):
    """anc0: the 0-based ancestors of all MANY_N slots"""
    want = many_tiles_reference()
    wrong = [(j, int(anc0[j]), a) for j, a in want.items() if a is not None and anc0[j] != a]
    assert not wrong, f"{len(wrong)} ancestors off the reference, first (slot, got, want) {wrong[:4]}"


def test_many_tiles_sampled(o):
    n = MANY_N
    T = o.targets_sorted(SEED, MANY_EPOCH, 0, n, n << 40)
    assert (np.diff(T.astype(np.int64)) >= 0).all()
    check_many_tiles(T >> np.uint64(40))                   # first a with (a + 1) 2^40 > T


# ------------------------------------------------------------------------------------------- negative controls
@functools.lru_cache(maxsize=None)
def _control_inputs(n, seed, slot0):
    sm = hw.Softmax(weight_vector("spread", n), hw.fix_K(n))
    return sm, hw.sorted_multinomial(sm, seed, RESAMPLE_EPOCH, slot0=slot0)


# mutation -> (n, seed, slot0): the attempt mutations on the case whose LAST tile rejects attempt 0 (one tile alone cancels out of V_t);
# the two id mutations on a view; what acts inside a tile at 65 slots, what acts on the totals at 2049
CONTROLS = {"attempt_blocks": REJECT_LAST + (0,), "accept_words23": REJECT_LAST + (0,), "last_shape": (2049, SEED, 0), "no_e_n": (65, SEED, 0),
            "tile_id_local": (2049, SEED, 5), "spacing_slot0": (2049, SEED, 5), "spacing_pair": (65, SEED, 0), "d_half": (2049, SEED, 0),
            "second_normal": (2049, SEED, 0), "exclusive": (65, SEED, 0), "boundary_next": (2049, SEED, 0)}


@pytest.mark.parametrize("mutation", hw.MUTATIONS)
def test_rejects(mutation):
    """the correct weights, the ancestors of the mutated construction: at least one decidable slot moved, and the checker says so"""
    n, seed, slot0 = CONTROLS[mutation]
    sm, good = _control_inputs(n, seed, slot0)
    assert not good.undecidable
    bad = hw.sorted_multinomial(sm, seed, RESAMPLE_EPOCH, slot0=slot0, mutate=mutation)
    moved = [j for j in range(n) if bad.anc[j] != good.anc[j] and j not in good.undecidable]
    assert moved, mutation
    with pytest.raises(AssertionError, match="ancestors off the reference"):
        hw.check_ancestors(good, np.array(bad.anc), sm, mutation)
    assert hw.check_ancestors(good, np.array(good.anc), sm, "the construction itself") == 0


def test_controls_cover_every_mutation():
    assert set(CONTROLS) == set(hw.MUTATIONS) and len(hw.MUTATIONS) == 11


if __name__ == "__main__":
    # the table "largest derived bound per quantity" of DESIGN.md 3.6: run the committed cases, print what the reference collected
    import sys
    rc = pytest.main([__file__, "-q", "-p", "no:cacheprovider"])
    for k, t in sorted(hw.SORTED_MAX.items()) + sorted(hc.MAX_TOL.items()):
        print(f"{k:60s} {t:.2g}")
    sys.exit(rc)
