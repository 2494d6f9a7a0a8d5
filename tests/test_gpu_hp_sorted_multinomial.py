"""The device filter's sorted multinomial resampler (GPF_RESAMPLE_MULTINOMIAL_SORTED) against tests/hp_weights.py's sorted_multinomial -- the
construction of DESIGN.md 3.6 in the reals, in mpmath -- through the drivers and checks of tests/test_hp_sorted_multinomial.py (there: the CPU
oracle).  Device == oracle is asserted bit for bit in tests/test_sorted_multinomial.py; this file is the device's own witness that gamma_tile,
spacing_of, the merge kernel's tile placement and k_sorted_tiles compute what the construction says: the tile totals drawn by a weight scan
of the call and in a launch of their own after a getter, pf_step_ess, views off the parent's tile grid, the uniform fallback, and 1025 tiles.
Every resample runs with check=False except test_invalid_weights_verdict.  No mutated kernel runs here (a corrupted value can
hang a look-back); the negative controls are on the CPU."""
import numpy as np
import pytest

import hp_checks as hc
import test_hp_sorted_multinomial as cpu
import test_hp_weights as weights

pytestmark = pytest.mark.gpu


@pytest.fixture
def device_run(g, o):
    """make_run on the device adapter; the states are closed whether the test passes or not"""
    made = []

    def make(n, name="lgssm2", **kw):
        r, ys = weights.make_run(hc.DeviceAdapter, g, o, n, name, **kw)
        made.append(r)
        return r, ys

    yield make
    for r in made:
        if r.a.st is not None:
            r.a.st.close()


@pytest.mark.parametrize("n,kind,alpha", cpu.GRID)
def test_resample(device_run, n, kind, alpha):
    r, ys = device_run(n)
    assert cpu.drive_case(r, ys, n, kind, alpha) == 0


@pytest.mark.parametrize("n,seed", cpu.REJECTED)
def test_rejected_first_attempt(device_run, n, seed):
    r, ys = device_run(n, seed=seed)
    assert cpu.drive_rejected(r, ys, n, seed) == 0


def test_invalid_weights_verdict(device_run):
    """check="warn", the synchronising path: the same checks, and the library's verdict `invalid` is the definition's"""
    r, ys = device_run(2049)
    r.a.check = "warn"
    assert cpu.drive_case(r, ys, 2049, "all_neginf", None) == 0
    r, ys = device_run(65)
    r.a.check = "warn"
    assert cpu.drive_case(r, ys, 65, "some_neginf", None) == 0


@pytest.mark.parametrize("name,n", [("lgssm2", 2049), ("bearings4", 1025)])
def test_log_ml_through_a_run(device_run, name, n):
    r, ys = device_run(n, name)
    cpu.drive_run(r, ys)


@pytest.mark.parametrize("n", [64, 2049])
def test_step_ess(device_run, n):
    r, ys = device_run(n)
    cpu.drive_step_ess(r, ys)


@pytest.mark.parametrize("sl,method", cpu.VIEW_CASES, ids=lambda v: v if isinstance(v, str) else f"{v.start}:{v.stop}:{v.step}")
def test_views(device_run, sl, method):
    r, ys = device_run(cpu.VIEW_N)
    assert cpu.drive_view(r, ys, sl, method) == 0


def test_view_under_a_priority(device_run):
    r, ys = device_run(cpu.VIEW_N)
    r.initialize(ys[0], check=False)
    r.update(ys[1], check=False)
    assert r.resample_view(cpu.VIEWS[1], cpu.SORTED, alpha=0.5) == 0
    r.update(ys[2])


def test_many_tiles_sampled(device_run):
    """1024 * 2048 + 1 particles of equal weight: 1025 tiles, placed by k_sorted_tiles and no longer by the merge kernel itself; the last
    tile holds one slot.  Ancestors of the five sampled tiles against the reference, the order over all slots, the gathered rows of the
    sampled tiles bit for bit.  The only test of this file above ~4100 particles."""
    n = cpu.MANY_N
    r, ys = device_run(n)
    r.initialize(ys[0], check=False)
    assert r.epoch == cpu.MANY_EPOCH
    r.a.set_lw(np.zeros(n))
    rows0 = r.a.rows
    r.a.resample(cpu.SORTED)
    anc0 = np.asarray(r.a.parents) - 1
    assert anc0.shape == (n,) and anc0.min() >= 0 and anc0.max() < n
    assert (np.diff(anc0) >= 0).all()
    cpu.check_many_tiles(anc0)
    rows = r.a.rows
    for t in cpu.MANY_TILES:
        sl = slice(t * 2048, min((t + 1) * 2048, n))
        assert np.array_equal(np.ascontiguousarray(rows[sl]).view(np.uint64), np.ascontiguousarray(rows0[anc0[sl]]).view(np.uint64)), t
    assert (r.a.lw == 0.0).all()
