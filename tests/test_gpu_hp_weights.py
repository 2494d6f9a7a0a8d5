"""The device filter's weight side against tests/hp_weights.py -- the definitions of the resamplers, of pf_resize, of the log-ML bookkeeping, of ESS
and of mean / var / proportionmap in mpmath on exact uniforms -- through the same cases and check functions as tests/test_hp_weights.py (there:
the CPU oracle).  Device == oracle is asserted bit for bit elsewhere; this file is the device's own witness that the scan, the reductions, the
searches, the gather, the weight update and the statistics kernels compute what the definitions say.  Every resample and resize runs with
check=False, the fully asynchronous path (all -Inf included: the uniform fallback's ancestors, rows, weights and log-ML = -Inf are checked, the
library reports no verdict there); test_all_neginf_verdict asks for the verdict through check="warn".  The optimal resize, pf_dereplicate
(method="sample"), pf_replicate, pf_coalesce and pf_introduce run the same drivers; the two optimal resizes with invalid weights run once more
with check="warn"."""
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


# ------------------------------------------------------------------------------------------- the rest of the resize family (resize.jl:149-334)
@pytest.mark.parametrize("n,n_new,kind,n_keep", cpu.OPTIMAL)
def test_optimal_resize(device_run, n, n_new, kind, n_keep):
    r, ys = device_run(n)
    assert cpu.drive_optimal(r, ys, n, n_new, kind, n_keep) == 0


@pytest.mark.parametrize("n,n_new,kind", cpu.OPTIMAL_INVALID)
def test_optimal_resize_invalid_verdict(device_run, n, n_new, kind):
    """check="warn": the library's verdict -- every weight -Inf, or every UNKEPT weight -Inf (the second scan) -- is the definition's"""
    r, ys = device_run(n)
    r.a.check = "warn"
    assert cpu.drive_optimal(r, ys, n, n_new, kind) == 0


@pytest.mark.parametrize("k,n_new,layout,kind", cpu.DEREPLICATE)
def test_dereplicate_sample(device_run, k, n_new, layout, kind):
    r, ys = device_run(k * n_new)
    assert cpu.drive_dereplicate(r, ys, k, n_new, layout, kind) == 0


@pytest.mark.parametrize("layout", ["contiguous", "interleaved"])
def test_replicate_round_trip(device_run, layout):
    r, ys = device_run(65)
    cpu.drive_replicate_round_trip(r, ys, layout)


@pytest.mark.parametrize("shape,n", cpu.COALESCE)
def test_coalesce_key_shapes(device_run, shape, n):
    r, ys = device_run(n)
    cpu.drive_coalesce(r, ys, shape, n)


def test_coalesce_after_a_resample(device_run):
    r, ys = device_run(2049)
    cpu.drive_coalesce_natural(r, ys, 2049)


@pytest.mark.parametrize("name,keep_prev", [("bearings4", True), ("sv1", False)])
def test_coalesce_by_a_column_and_the_padding(device_run, name, keep_prev):
    r, ys = device_run(2049, name)
    cpu.drive_coalesce_by_column(r, ys, 2049, keep_prev)


@pytest.fixture
def device_intro_run(g, o):
    made = []

    def make(name, n):
        r, ys = cpu.make_intro_run(hc.DeviceAdapter, g, o, name, n)
        made.append(r)
        return r, ys

    yield make
    for r in made:
        if r.a.st is not None:
            r.a.st.close()


@pytest.mark.parametrize("name,T,proposal,sizes", cpu.INTRODUCE)
def test_introduce(device_intro_run, name, T, proposal, sizes):
    r, ys = device_intro_run(name, sizes[0])
    cpu.drive_introduce(r, ys, T, sizes[1], proposal)


@pytest.mark.parametrize("after_resample,twice", [(True, False), (False, True)])
def test_introduce_after_a_resample_and_twice(device_intro_run, after_resample, twice):
    r, ys = device_intro_run("lgssm2", 65)
    cpu.drive_introduce(r, ys, 2, 257, after_resample=after_resample, twice=twice)
