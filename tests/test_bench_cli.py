"""bench.py's command line, on the CPU: main() runs against a stand-in for `gpf_amd` (same host interface, the
oracle underneath, fake kernel timers) with the driver's own flags and with degenerate ones, and must print exactly
ONE JSON line: with --full carrying `roofline` and `cpu_baseline`, without it only the headline (W + K steps, nothing
else).  Round 1's bench indexed observations past the end whenever --steps + --warmup < 30 (the gather and cpu_baseline
legs run a fixed number of steps); this keeps that from coming back.
The real library path of the same command is covered by tests/test_gpu_bench_cli.py on the GPU box."""
import importlib
import io
import json
import sys
import types
from contextlib import redirect_stdout

import numpy as np
import pytest


class _FakeState:
    """What bench.py touches on a DeviceParticleFilterState."""

    def __init__(self, o, model, obs, n, seed):
        self.orc = o.OracleFilter(model.model_id, model.params, n, seed).initialize(obs)
        self.row_width = model.row_width(False)
        self.n_particles = n
        self.updates = 0
        self._timing = {}
        self._count = {}

    @property
    def traces(self):
        return self.orc.rows.copy()

    @property
    def log_weights(self):
        return self.orc.lw.copy()

    @property
    def parents(self):
        return self.orc.parents - 1                # the oracle keeps Julia's 1-based ids

    def synchronize(self):
        pass

    def kernel_timing(self, kid, on):
        self._timing[kid] = bool(on)
        if on:
            self._count[kid] = 0

    def kernel_time(self, kid):
        c = self._count.get(kid, 0)
        return 0.02 * c, c                         # 20 us per launch

    def _launched(self, *kids):
        for k in kids:
            if self._timing.get(k):
                self._count[k] = self._count.get(k, 0) + 1


def _install_stub(monkeypatch, o):
    import gpf_amd as real
    stub = types.ModuleType("gpf_amd")
    stub.models, stub._lib = real.models, real._lib
    L = real._lib

    def pf_initialize(model, args, obs, n, seed=1, device=0):
        stub.last_state = _FakeState(o, model, obs, n, seed)
        return stub.last_state

    def pf_resample(state, method="multinomial", check="warn", **kw):
        state.orc.resample(method, check=False, **kw)
        state._launched(L.K_SCAN, L.K_SEARCH)
        state.pending = True

    def pf_update(state, args, argdiffs, obs):
        state.orc.update(np.asarray(obs, float))
        state.updates += 1
        state._launched(L.K_STEP)
        state.pending = False

    def get_ess(state):
        if getattr(state, "pending", False):
            state._launched(L.K_GATHER)
            state.pending = False
        return state.orc.effective_sample_size()

    def get_lml_est(state):
        return state.orc.log_ml_estimate()

    for f in (pf_initialize, pf_resample, pf_update, get_ess, get_lml_est):
        setattr(stub, f.__name__, f)
    monkeypatch.setitem(sys.modules, "gpf_amd", stub)
    import torch
    monkeypatch.setattr(torch.cuda, "set_device", lambda *_a, **_k: None)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *_a, **_k: None)
    return stub


def _run_main(monkeypatch, argv):
    """bench.main() with `argv` (512 particles): the one stdout line as a dict"""
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "GPF_BENCH_FORCE_SHARDED", "GPF_BENCH_ONE_DEVICE"):
        monkeypatch.delenv(k, raising=False)
    bench = importlib.import_module("bench")
    monkeypatch.setattr(sys, "argv", ["bench.py", "--particles-per-gpu", "512"] + argv)
    buf = io.StringIO()
    with redirect_stdout(buf):
        bench.main()
    lines = [ln for ln in buf.getvalue().splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


@pytest.mark.parametrize("argv", [
    ["--gpus", "1", "--steps", "20", "--warmup", "5"],          # the driver's command line (BENCH_r01 crashed on it)
    ["--steps", "1", "--warmup", "0"],
    ["--steps", "3", "--warmup", "40"],
    ["--steps", "100", "--warmup", "2"],
])
def test_bench_main_prints_one_json_line(argv, o, built, monkeypatch):
    _install_stub(monkeypatch, o)
    out = _run_main(monkeypatch, argv + ["--full"])
    steps = int(argv[argv.index("--steps") + 1])
    assert out["steps"] == steps and out["n_gpus"] == 1 and out["unit"] == "particle-steps/sec"
    assert out["dtype"] == "f64" and out["higher_is_better"] is True and out["vs_baseline"] is None
    assert "configs[1]" in out["config"]["workload"] and "model" not in out["config"]
    assert out["value"] > 0 and out["ms_per_step"] > 0
    r = out["roofline"]
    assert r is not None and r["bound"] == "hbm" and r["peak"] == 8000.0 and 0 < r["frac"] < 1 and "traffic" in r
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    assert r["traffic_source"] is not None and (r["traffic"] is None) == isinstance(r["traffic_source"], str)   # a figure only with its provenance
    c = out["cpu_baseline"]
    assert c is not None and c["kind"] == "port" and c["cores"] == 1 and c["value"] > 0 and c["sample"]
    assert set(out["resample_gather_kernel"]) == {"multinomial", "multinomial_sorted", "stratified"}
    sv = out["multinomial_sorted_variant"]                          # the opt-in sorted multinomial as a named variant beside the unchanged headline
    assert sv is not None and sv["value"] > 0 and "multinomial_sorted" in sv["workload"] and "configs[1]" in out["config"]["workload"]
    ss = out["stratified_sort_particles_variant"]                   # :stratified with the reference's default sort_particles=true
    assert ss is not None and ss["value"] > 0 and "sort_particles=true" in ss["workload"]
    assert np.isfinite(out["log_ml_estimate"]) and np.isfinite(out["log_ml_abs_error"])


@pytest.mark.parametrize("argv", [["--gpus", "1", "--steps", "20", "--warmup", "5"], ["--steps", "1", "--warmup", "0"]])
def test_plain_run_is_the_headline_and_dumps_its_outputs(argv, o, built, monkeypatch, tmp_path):
    """without --full: exactly W + K filter steps, the extra legs null; --dump-outputs writes the state after the last timed step,
    the same arrays a --full run of the same arguments writes before its extra legs move the filter on"""
    stub = _install_stub(monkeypatch, o)
    steps, warmup = int(argv[argv.index("--steps") + 1]), int(argv[argv.index("--warmup") + 1])
    out = _run_main(monkeypatch, argv + ["--dump-outputs", str(tmp_path / "plain")])
    st = stub.last_state
    assert st.updates == warmup + steps
    assert out["steps"] == steps and out["warmup"] == warmup and out["n_gpus"] == 1
    assert out["metric"] == out["unit"] == "particle-steps/sec" and out["higher_is_better"] is True and out["dtype"] == "f64"
    assert out["value"] > 0 and out["ms_per_step"] > 0
    assert abs(out["value"] - 512 * 1e3 / out["ms_per_step"]) < 1e-2 * out["value"]          # (ms_per_step is rounded)
    for k in ("roofline", "cpu_baseline", "cpu_baseline_multithread", "resample_gather_kernel", "multinomial_sorted_variant",
              "stratified_sort_particles_variant", "log_ml_exact_kalman", "log_ml_abs_error"):
        assert out[k] is None, k
    d = tmp_path / "plain"
    names = {"traces", "log_weights", "parents", "log_ml_estimate"}
    assert {f.name for f in d.iterdir()} == {n + ".npy" for n in names}
    got = {n: np.load(d / (n + ".npy")) for n in names}
    assert all(a.dtype == np.float64 for a in got.values())
    np.testing.assert_array_equal(got["traces"], st.orc.rows)
    np.testing.assert_array_equal(got["log_weights"], st.orc.lw)
    np.testing.assert_array_equal(got["parents"], st.orc.parents - 1)
    assert got["log_ml_estimate"].tolist() == [out["log_ml_estimate"]] == [st.orc.log_ml_estimate()]
    full = _run_main(monkeypatch, argv + ["--full", "--no-cpu-baseline", "--dump-outputs", str(tmp_path / "full")])
    assert full["roofline"] is not None and full["log_ml_estimate"] == out["log_ml_estimate"]
    for n in names:
        np.testing.assert_array_equal(np.load(tmp_path / "full" / (n + ".npy")), got[n])


def test_dump_outputs_keeps_a_seeded_sample_within_the_budget(monkeypatch, tmp_path):
    """over the byte budget every array keeps the same fixed sample of particles, and the indices are written beside them"""
    bench = importlib.import_module("bench")
    monkeypatch.setattr(bench, "DUMP_BYTES", 64_000)
    n = 10_000

    class _State:
        n_particles = n
        traces = np.arange(2 * n, dtype=np.float64).reshape(n, 2)
        log_weights = -np.arange(n, dtype=np.float64)
        parents = np.arange(n, dtype=np.int64)[::-1].copy()
    for sub in ("a", "b"):
        bench.dump_outputs(str(tmp_path / sub), _State(), -1.5, 0, 1)
    total = sum(f.stat().st_size for f in (tmp_path / "a").iterdir())
    assert 0.99 * 64_000 < total <= 64_000                              # (.npy headers included)
    idx = np.load(tmp_path / "a" / "sample_index.npy")
    assert 0 < idx.size < n and np.all(np.diff(idx) > 0)
    i = idx.astype(np.int64)
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "traces.npy"), _State.traces[i])
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "log_weights.npy"), _State.log_weights[i])
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "parents.npy"), _State.parents[i])
    for f in (tmp_path / "a").iterdir():
        np.testing.assert_array_equal(np.load(f), np.load(tmp_path / "b" / f.name))
    # one of two ranks: its own shard, named by rank, within half the budget
    bench.dump_outputs(str(tmp_path / "r"), _State(), -1.5, 1, 2)
    names = {"traces", "log_weights", "parents", "sample_index", "log_ml_estimate"}
    assert {f.name for f in (tmp_path / "r").iterdir()} == {n + "_rank1.npy" for n in names}
    assert sum(f.stat().st_size for f in (tmp_path / "r").iterdir()) <= 64_000 // 2


# ---- `python bench.py --gpus N` with no WORLD_SIZE: the launcher branch (the driver's scaling command; round 2 exited rc 1 on it)
def _fake_torchrun(tmp_path, body):
    """a stand-in for `python -m torch.distributed.run` on sys.path of the child: records its argv, then runs `body`"""
    pkg = tmp_path / "torch" / "distributed"
    pkg.mkdir(parents=True)
    (tmp_path / "torch" / "__init__.py").write_text("")
    (pkg / "__init__.py").write_text("")
    (pkg / "run.py").write_text("import sys, json, os, time\nargv = sys.argv[1:]\n" + body)
    return str(tmp_path)


def _run_launcher(tmp_path, body, extra=()):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=_fake_torchrun(tmp_path, body))
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    return subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "20", "--warmup", "5", *extra],
                          capture_output=True, text=True, env=env, timeout=120)


def test_launcher_starts_ranks_and_relays_the_json_line(tmp_path):
    body = ("print('RCCL version banner')\n"
            "assert '--nproc-per-node' in argv and argv[argv.index('--nproc-per-node') + 1] == '2', argv\n"
            "assert '--master-addr' in argv and argv[argv.index('--master-addr') + 1] == '127.0.0.1'\n"
            "assert argv[-6:] == ['--gpus', '2', '--steps', '20', '--warmup', '5'], argv\n"
            "assert os.environ.get('HSA_ENABLE_IPC_MODE_LEGACY') == '0'\n"
            "print(json.dumps({'metric': 'particle-steps/sec', 'value': 1.0, 'n_gpus': 2}))\n"
            "print('trailing noise')\n")
    p = _run_launcher(tmp_path, body)
    assert p.returncode == 0, p.stderr
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 1 and json.loads(lines[0])["n_gpus"] == 2          # the JSON line is the only (so the last) stdout line
    assert "RCCL version banner" in p.stderr and "trailing noise" in p.stderr


def test_launcher_hands_the_ranks_an_absolute_dump_directory(tmp_path):
    """the ranks start in the repository root: a relative --dump-outputs DIR reaches them as the directory the caller meant"""
    import os
    want = os.path.abspath("dumps")                                   # (the launcher runs in this process's directory)
    body = (f"assert argv[-2:] == ['--dump-outputs', {want!r}], argv\n"
            "print(json.dumps({'metric': 'particle-steps/sec', 'value': 1.0, 'n_gpus': 2}))\n")
    p = _run_launcher(tmp_path, body, extra=("--dump-outputs", "dumps"))
    assert p.returncode == 0, p.stderr


def test_launcher_propagates_a_rank_failure(tmp_path):
    p = _run_launcher(tmp_path, "print('rank 1 died', file=sys.stderr)\nsys.exit(3)\n")
    assert p.returncode == 3 and p.stdout.strip() == ""


def test_launcher_needs_a_json_line(tmp_path):
    p = _run_launcher(tmp_path, "print('no result')\n")
    assert p.returncode != 0 and "without a JSON line" in p.stderr


def test_launcher_kills_a_hung_job(tmp_path):
    import time
    t0 = time.time()
    p = _run_launcher(tmp_path, "time.sleep(600)\n", extra=("--launch-timeout", "3"))
    assert p.returncode == 124 and time.time() - t0 < 60 and "killed" in p.stderr


def test_rank_count_mismatch_is_an_error(monkeypatch, built):
    monkeypatch.setenv("WORLD_SIZE", "1")
    bench = importlib.import_module("bench")
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2"])
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert "WORLD_SIZE=1" in str(e.value)
