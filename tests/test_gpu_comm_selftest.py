"""c2r_comm_selftest, C2R_COMM_SELFTEST, c2r_get_comm_timing and tools/comm_firstcontact.py on the ONE device of the GPU box.

The sums are carried by the stand-in for librccl (tests/fake_rccl.hip) -- and by a second one that LIES on request
(tests/fake_rccl_corrupt.hip: a flipped bit, a reduction through fp32, a rank whose sum never arrived): an honest transport
must pass, every kind of lie must be named.  One short-lived worker process per library and corruption mode
(tests/comm_selftest_worker.py; the library binds its RCCL once per process), one after another, each under a time limit; the
worker asserts what it sees and this file what it wrote.  The last two tests wait for a box with two devices: they are what
such a box should run first."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
LOGS = os.environ.get("C2R_TEST_LOG_DIR")   # where the workers' output is kept; unset: next to their results (pytest's tmp)
WORKER = ROOT / "tests" / "comm_selftest_worker.py"
TOOL = ROOT / "tools" / "comm_firstcontact.py"
DROP = ("C2R_FAULT_INJECT", "FAKE_RCCL_HANG", "C2R_COMM_TIMEOUT_S", "FAKE_RCCL_CORRUPT", "C2R_COMM_SELFTEST", "FAKE_RCCL_MULTIPROCESS",
        "C2R_RCCL_LIBRARY", "C2R_COMM_SHARED_DEVICE_RCCL", "WORLD_SIZE", "RANK", "LOCAL_RANK", "C2R_ALLREDUCE_SLABS")


def build_standin(name):
    """tests/_<name>.so from tests/<name>.hip, on demand (the lying one includes the honest one)"""
    src, so = ROOT / "tests" / f"{name}.hip", ROOT / "tests" / f"_{name}.so"
    newest = max(p.stat().st_mtime for p in (src, ROOT / "tests" / "fake_rccl.hip"))
    if not so.exists() or so.stat().st_mtime < newest:
        subprocess.run(["hipcc", "--offload-arch=gfx950", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-std=c++17", "-pthread",
                        "-o", str(so), str(src)], check=True)
    return so


def base_env(library=None, **extra):
    env = {k: v for k, v in os.environ.items() if k not in DROP}
    if library:
        env.update(C2R_RCCL_LIBRARY=str(build_standin(library)), C2R_COMM_SHARED_DEVICE_RCCL="1", FAKE_RCCL_TIMEOUT_S="60")
    env.update(extra)
    return env


def log_dir(fallback):
    d = Path(LOGS) if LOGS else Path(fallback)
    d.mkdir(parents=True, exist_ok=True)
    return d


def log(name, r, fallback):
    (log_dir(fallback) / f"comm_selftest_{name}.log").write_text(r.stdout[-20000:] + "\n--- stderr ---\n" + r.stderr[-20000:])


def run_worker(mode, out, env, timeout=300):
    r = subprocess.run([sys.executable, str(WORKER), mode, str(out)], env=env, capture_output=True, text=True, timeout=timeout)
    log(out.name, r, out.parent)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return json.loads((out / f"{mode}.json").read_text()), r


def run_pair(mode, out, env, extra, timeout=240):
    """two worker processes at a time (ranks 0 and 1), each under the time limit"""
    procs = [subprocess.Popen([sys.executable, str(WORKER), mode, str(out), str(r), str(extra[r])], env=env, stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE, text=True) for r in range(2)]
    res = []
    try:
        for p in procs:
            so, se = p.communicate(timeout=timeout)
            res.append((p.returncode, so, se))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    (log_dir(out.parent) / f"comm_selftest_{out.name}.log").write_text("\n".join(f"--- rank {r}: status {c}\n{so[-8000:]}\n{se[-8000:]}" for r, (c, so, se) in enumerate(res)))
    assert [c for c, _, _ in res] == [0, 0], "\n".join(so[-1500:] + se[-1500:] for _, so, se in res)
    return [json.loads((out / f"{mode}_rank{r}.json").read_text()) for r in range(2)]


@pytest.fixture(scope="module")
def honest(tmp_path_factory):
    out = tmp_path_factory.mktemp("honest")
    summary, r = run_worker("honest", out, base_env("fake_rccl"), timeout=600)
    return out, summary, r


def test_honest_standin_passes_in_one_process(honest):
    """c2r_create_multi([0] * n) + c2r_comm_init_local, n = 2, 4, 8, on a context fresh from create, an isothermal and a heating
    one: 0, ranks == n, nothing mismatched, rates_count and ncomp * ncell + 48 doubles compared -- and the stand-in's counters
    show that it launched exactly the collectives of the two routes (the worker compares them around every call)."""
    _, s, _ = honest
    assert s["library"].endswith("_fake_rccl.so"), s["library"]
    ncell = 16 ** 3
    for n in (2, 4, 8):
        for name, ncomp in (("fresh", 3), ("iso", 3), ("heat", 4)):
            rep = s[f"multi_{name}_N{n}"]
            assert rep["ranks"] == n and rep["devices"] == n and rep["kind"] == 1 and rep["mismatches"] == [0, 0], rep
            assert rep["elements"] == [4 * ncell + 48, ncomp * ncell + 48], rep
    cliques, calls, launched, largest = s["stats"]
    assert largest == 8 and launched >= 9 * 14 and calls > 2 * launched, s["stats"]


def test_honest_standin_passes_with_a_context_per_rank(honest):
    """c2r_create + c2r_comm_init on a host thread per rank, n = 2, 3: every rank's own verdict"""
    _, s, _ = honest
    for n in (2, 3):
        for name, ncomp in (("fresh", 3), ("heat", 4)):
            reps = s[f"threads_{name}_N{n}"]
            assert len(reps) == n
            for rep in reps:
                assert rep["ranks"] == n and rep["devices"] == 1 and rep["mismatches"] == [0, 0] and rep["elements"][1] == ncomp * 16 ** 3 + 48, rep


def test_honest_standin_passes_in_two_processes(tmp_path):
    out = tmp_path / "mp_honest"
    reps = run_pair("mp", out, base_env("fake_rccl", FAKE_RCCL_MULTIPROCESS="1"), extra=[0, 0])
    for r in reps:
        assert r["report"]["ranks"] == 2 and r["report"]["mismatches"] == [0, 0] and r["library"].endswith("_fake_rccl.so"), r


def test_shared_device_sum_and_contexts_without_communicator(honest):
    _, s, _ = honest
    assert s["kind2"]["kind"] == 2 and s["kind2"]["ranks"] == 2 and s["kind2"]["mismatches"] == [0, 0], s["kind2"]
    assert s["single"]["ranks"] == 1 and s["single"]["elements"] == [0, 0], s["single"]
    assert "a multi-device context needs c2r_comm_init_local or c2r_comm_init first" in s["multi_no_comm"]


@pytest.mark.parametrize("lie", ["bitflip:1:1:1234", "bitflip:0:7:77", "fp32", "stale:1"])
def test_lies_are_caught(tmp_path, lie):
    """Each lie in a fresh worker with the lying library, n = 2 and 4 (the worker asserts the details: exactly one mismatch at
    the rank and index asked for and one differing bit; every element of every rank on both routes; rank 1's device alone)."""
    out = tmp_path / ("lie_" + lie.replace(":", "_"))
    s, _ = run_worker("lie", out, base_env("fake_rccl_corrupt", FAKE_RCCL_CORRUPT=lie))
    for n in ("2", "4"):
        c = s["cases"][n]
        assert "WRONG" in c["message"] and s["library"] in c["message"] and sum(c["report"]["mismatches"]) > 0, c
        assert "was aborted after an earlier error" in c["again"], c
    if lie == "fp32":   # the switch at communicator set-up made the difference (test 6)
        assert "WRONG" in s["init_local"] and all("WRONG" in x for x in s["init_rank"]), s


def test_lying_library_is_transparent_when_not_asked_to_lie(honest, tmp_path):
    out = tmp_path / "transparent"
    run_worker("transparent", out, base_env("fake_rccl_corrupt"))
    ref, got = np.load(honest[0] / "honest_heat16_N2.npz"), np.load(out / "transparent_heat16_N2.npz")
    assert len(got.files) >= 10
    for k in got.files:
        assert np.array_equal(got[k], ref[k]), k


def test_selftests_do_not_change_a_run(honest):
    """three fused and three plain iterations with a self-test before begin_step and between the iterations: every grid, conv,
    photon_loss and sum_nbox bit-identical to the run without (compared in the worker)"""
    _, s, _ = honest
    for tag in ("fused", "plain"):
        for k in ("phih_grid", "phihe_grid", "phiheat", "xh_av", "xhe_av", "xh_intermed", "xhe_intermed", "photon_loss", "sum_nbox", "conv"):
            assert f"{tag}_{k}" in s["non_interference_keys"]


def test_switch_at_communicator_setup_prints_ok(honest):
    _, _, r = honest
    ok = [line for line in r.stderr.splitlines() if line.startswith("c2ray_hip: comm self-test ok: 2 ranks")]
    assert len(ok) == 3 and all("_fake_rccl.so" in line and " ms" in line for line in ok), r.stderr[-2000:]   # init_local once, init on two ranks


def test_rcclcomm_selftest_agrees_over_gloo(tmp_path):
    """two processes, gloo for the agreement, the lying stand-in with stale:1: BOTH ranks raise the same text"""
    out = tmp_path / "gloo_stale"
    port = 29500 + (os.getpid() % 2000)
    res = run_pair("gloo", out, base_env("fake_rccl_corrupt", FAKE_RCCL_MULTIPROCESS="1", FAKE_RCCL_CORRUPT="stale:1"), extra=[port, port])
    assert res[0]["error"] and res[0]["error"] == res[1]["error"], res
    assert res[0]["error"].startswith("comm self-test failed: rank "), res


def test_comm_timing(honest):
    _, s, _ = honest
    for n in ("2", "4"):
        rows = s["timing"][n]
        assert len(rows) == 2 * int(n)
        for ct in rows:
            assert ct["slabs"] == 3 and ct["tail_ms"] >= 0 and 0 <= ct["allreduce_exposed_ms"] <= ct["allreduce_ms"] < ct["wall_ms"], ct
    assert s["timing_no_comm"] == {"slabs": 0, "allreduce_ms": 0.0, "allreduce_exposed_ms": 0.0, "tail_ms": 0.0}


def test_firstcontact_tool(tmp_path):
    cmd = [sys.executable, str(TOOL), "--gpus", "2", "--mesh", "32", "--steps", "2", "--share-device"]
    r = subprocess.run(cmd, env=base_env("fake_rccl"), capture_output=True, text=True, timeout=300)
    log("firstcontact", r, tmp_path)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["ok"] and "STAND-IN" in d["transport"] and d["rccl_ranks"] == 0 and d["library"].endswith("_fake_rccl.so"), d
    assert d["selftest"]["ranks"] == 2 and d["selftest"]["mismatches"] == [0, 0] and d["ms_per_step"] > 0
    assert len(d["devices"]) == 2
    keys = ("sweep_ms", "rates_ms", "chem_ms", "allreduce_ms", "allreduce_exposed_ms", "tail_ms")
    for row in d["devices"]:
        assert row["slabs"] == 4 and all(row[k] >= 0 for k in keys), row
    for k in keys:
        assert set(d["over_devices"][k]) == {"max", "mean", "max_over_mean"}
    r = subprocess.run(cmd, env=base_env("fake_rccl_corrupt", FAKE_RCCL_CORRUPT="fp32"), capture_output=True, text=True, timeout=300)
    log("firstcontact_fp32", r, tmp_path)
    assert r.returncode != 0 and "ms_per_step" not in r.stdout and "WRONG" in r.stdout + r.stderr, r.stdout[-2000:] + r.stderr[-2000:]


def _two_devices():
    import torch
    return torch.cuda.is_available() and torch.cuda.device_count() >= 2


@pytest.mark.skipif(not _two_devices(), reason="needs two HIP devices (the real RCCL refuses ranks that share one)")
def test_real_rccl_selftest_one_process(tmp_path):
    s, _ = run_worker("real_local", tmp_path / "real_local", base_env())
    assert os.path.basename(s["library"]).startswith("librccl") and s["report"]["mismatches"] == [0, 0], s


@pytest.mark.skipif(not _two_devices(), reason="needs two HIP devices (the real RCCL refuses ranks that share one)")
def test_real_rccl_selftest_two_processes(tmp_path):
    reps = run_pair("mp", tmp_path / "real_mp", base_env(), extra=[0, 1])
    for r in reps:
        assert os.path.basename(r["library"]).startswith("librccl") and r["report"]["mismatches"] == [0, 0], r
