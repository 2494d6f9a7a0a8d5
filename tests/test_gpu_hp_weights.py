"""The device filter's weight side against tests/hp_weights.py -- the definitions of the resamplers, of pf_resize, of the log-ML bookkeeping, of ESS
and of mean / var / proportionmap in mpmath on exact uniforms -- through the same cases and check functions as tests/test_hp_weights.py (there:
the CPU oracle).  Device == oracle is asserted bit for bit elsewhere; this file is the device's own witness that the scan, the reductions, the
searches, the gather, the weight update and the statistics kernels compute what the definitions say.  Every resample and resize runs with
check=False, the fully asynchronous path (all -Inf included: the uniform fallback's ancestors, rows, weights and log-ML = -Inf are checked, the
library reports no verdict there); test_all_neginf_verdict asks for the verdict through check="warn"."""
import pytest

import hp_checks as hc
import test_hp_weights as cpu

pytestmark = pytest.mark.gpu


@pytest.fixture
def device_run(g, o):
    """make_run on the device adapter; the states are closed whether the test passes or not"""
    made = []

    def make(n, name="lgssm2", **kw):
        r, ys = cpu.make_run(hc.DeviceAdapter, g, o, n, name, **kw)
        made.append(r)
        return r, ys

    yield make
    for r in made:
        if r.a.st is not None:
            r.a.st.close()


@pytest.mark.parametrize("n,kind,form,alpha", cpu.GRID)
def test_resample(device_run, n, kind, form, alpha):
    r, ys = device_run(n)
    assert cpu.drive_case(r, ys, n, kind, form, alpha) == 0


@pytest.mark.parametrize("form", cpu.FORMS)
def test_all_neginf_verdict(device_run, form):
    """check="warn", the synchronising path: the same checks, and the library's verdict `invalid` is the definition's"""
    r, ys = device_run(2049)
    r.a.check = "warn"
    assert cpu.drive_case(r, ys, 2049, "all_neginf", form, None) == 0
    r, ys = device_run(65)
    r.a.check = "warn"
    assert cpu.drive_case(r, ys, 65, "some_neginf", form, None) == 0


@pytest.mark.parametrize("name,n", [("lgssm2", 2049), ("bearings4", 1025)])
def test_log_ml_through_a_run(device_run, name, n):
    r, ys = device_run(n, name)
    cpu.drive_run(r, ys)


@pytest.mark.parametrize("n", [65, 2049])
def test_statistics_of_current_and_past_addresses(device_run, n):
    r, ys = device_run(n, "object_motion", history=True)
    cpu.drive_history(r, ys)


@pytest.mark.parametrize("n", [64, 1025, 2049])
def test_step_ess_verdict(device_run, n):
    r, ys = device_run(n)
    cpu.drive_step_ess(r, ys)


@pytest.mark.parametrize("nb", cpu.BLOCK_SIZES)
def test_block_estimates(device_run, nb):
    n_blocks = 3 if nb == 2048 else 4
    r, ys = device_run(nb * n_blocks, "object_motion")
    cpu.drive_blocks(r, ys, nb, n_blocks)


@pytest.mark.parametrize("n_new,method,alpha", cpu.RESIZES)
def test_resize(device_run, n_new, method, alpha):
    r, ys = device_run(2049)
    assert cpu.drive_resize(r, ys, n_new, method, alpha) == 0


def test_sample_unweighted(device_run):
    r, ys = device_run(2049)
    r.initialize(ys[0], check=False)
    r.update(ys[1], check=False)
    assert r.sample_unweighted(65) == 0
    r.update(ys[2])
