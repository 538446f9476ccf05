"""TEST INFRASTRUCTURE ONLY: c2r_comm_selftest, C2R_COMM_SELFTEST and c2r_get_comm_timing through a stand-in for librccl
(tests/fake_rccl.hip, or tests/fake_rccl_corrupt.hip which returns wrong sums on request).  Run by
tests/test_gpu_comm_selftest.py, one short-lived process per library and corruption mode -- the library binds its RCCL once
per process:

    python tests/comm_selftest_worker.py MODE OUTDIR [RANK [PORT|DEVICE]]

MODE: honest | lie | transparent | mp | gloo | real_local.  Asserts what it can see itself and writes OUTDIR/<mode>.json (and
.npz files the parent test compares across workers); exit status 0 means every assertion here held."""
import ctypes as C
import dataclasses
import json
import os
import sys
import threading
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

from rccl_standin_worker import case_heating16, engine  # noqa: E402

NSLAB = 4
GRIDS = ("phih_grid", "phihe_grid", "phiheat", "xh_av", "xhe_av", "xh_intermed", "xhe_intermed", "photon_loss", "sum_nbox", "conv")


def stats(fake):
    s = (C.c_longlong * 4)()
    fake.fake_rccl_stats(s)
    return list(s)


def check_ok(rep, n, ncell, ncomp, devices, kind=1):
    assert rep["ranks"] == n and rep["kind"] == kind and rep["devices"] == devices, rep
    assert rep["mismatches"] == [0, 0] and rep["bad_route"] == -1 and rep["bad_rank"] == -1 and rep["bad_index"] == -1, rep
    assert rep["elements"] == [4 * ncell + 48, ncomp * ncell + 48], rep
    assert rep["ms"][0] >= 0 and rep["ms"][1] >= 0, rep


def iso_case(case):
    mesh, mat, grid, src, cosmo, dt = case
    return mesh, dataclasses.replace(mat, isothermal=True, temperature_grid=None), grid, src, cosmo, dt


def run_iterations(e, dt, fused, plain, selftests):
    """begin_step, `fused` fused and `plain` plain iterations; a self-test before begin_step and between the iterations."""
    out = {}
    if selftests:
        e.comm_selftest(NSLAB)
    e.begin_step()
    conv = []
    for it in range(fused + plain):
        if selftests and it > 0:
            e.comm_selftest(NSLAB)
        e.set_rates_to_zero()
        if it < fused:
            conv.append(e.pass_allreduce_chemistry(dt, 1, 1, 3))
        else:
            e.pass_sources(1, 1)
            e.allreduce_rates()
            conv.append(e.global_pass(dt))
        if it + 1 in (fused, fused + plain):
            tag = "fused" if it + 1 == fused else "plain"
            for k, v in {**e.download_rates(), **e.download_iter_state(), "conv": np.array(conv)}.items():
                out[f"{tag}_{k}"] = np.asarray(v).copy()
    return out


def threads_selftest(pkg, tables, case, n, upload=True):
    """a context per rank, each on a host thread of its own (c2r_comm_init): every rank's report, or its error"""
    uid = pkg.HipEngine.comm_unique_id()
    rep, err = [None] * n, [None] * n

    def body(r):
        try:
            e = engine(pkg, tables, case, 0, upload=upload)
            e.comm_init(r, n, uid)
            rep[r] = e.comm_selftest(NSLAB)
            e.close()
        except Exception as ex:  # noqa: BLE001 -- reported to the caller
            err[r] = f"{type(ex).__name__}: {ex}"

    th = [threading.Thread(target=body, args=(r,)) for r in range(n)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    return rep, err


def mode_honest(pkg, tables, out, summary):
    fake = C.CDLL(os.environ["C2R_RCCL_LIBRARY"])
    heat16 = case_heating16(pkg)
    iso16 = iso_case(heat16)
    mesh, dt = heat16[0], heat16[5]
    ncell = int(np.prod(mesh))
    summary["library"] = pkg.HipEngine.comm_library()
    # 1. one process, n communicators: fresh from create, isothermal, heating
    for n in (2, 4, 8):
        for name, ncomp in (("fresh", 3), ("iso", 3), ("heat", 4)):
            s0 = stats(fake)
            if name == "fresh":
                e = pkg.HipEngine(mesh, [0] * n)
            else:
                e = engine(pkg, tables, iso16 if name == "iso" else heat16, [0] * n)
            e.comm_init_local()
            rep = e.comm_selftest(NSLAB)
            check_ok(rep, n, ncell, ncomp, n)
            s1 = stats(fake)
            per_rank = 1 + NSLAB * ncomp + 1          # whole buffer, the slabs' component ranges, the tail
            assert s1[2] - s0[2] == per_rank and s1[1] - s0[1] == n * per_rank, (s0, s1, n, name)
            summary[f"multi_{name}_N{n}"] = rep
            if name == "heat":                       # ... and the context still does its work afterwards
                e.begin_step()
                e.set_rates_to_zero()
                e.pass_allreduce_chemistry(dt, 1, 1, 3)
            e.close()
    # a context per rank on its own thread
    for n in (2, 3):
        for name, case, ncomp in (("fresh", None, 3), ("heat", heat16, 4)):
            if case is None:
                uid = pkg.HipEngine.comm_unique_id()
                rep, err = [None] * n, [None] * n

                def body(r):
                    try:
                        e = pkg.HipEngine(mesh, 0)
                        e.comm_init(r, n, uid)
                        rep[r] = e.comm_selftest(NSLAB)
                        e.close()
                    except Exception as ex:  # noqa: BLE001
                        err[r] = str(ex)
                th = [threading.Thread(target=body, args=(r,)) for r in range(n)]
                [t.start() for t in th]
                [t.join() for t in th]
            else:
                rep, err = threads_selftest(pkg, tables, case, n)
            assert not any(err), err
            for r in range(n):
                check_ok(rep[r], n, ncell, ncomp, 1)
            summary[f"threads_{name}_N{n}"] = rep
    summary["stats"] = stats(fake)
    # 2. kind 2 (replicas share a device, no RCCL); no communicator
    shared = os.environ.pop("C2R_COMM_SHARED_DEVICE_RCCL")
    e = engine(pkg, tables, heat16, [0, 0])
    e.comm_init_local()
    rep = e.comm_selftest(NSLAB)
    check_ok(rep, 2, ncell, 4, 2, kind=2)
    summary["kind2"] = rep
    e.close()
    os.environ["C2R_COMM_SHARED_DEVICE_RCCL"] = shared
    e = engine(pkg, tables, heat16, 0)
    rep = e.comm_selftest(NSLAB)
    assert rep["ranks"] == 1 and rep["elements"] == [0, 0] and rep["mismatches"] == [0, 0] and rep["kind"] == 0, rep
    summary["single"] = rep
    # (7: a context without communicator has no comm timing)
    e.enable_timing(True)
    e.begin_step()
    e.set_rates_to_zero()
    e.pass_allreduce_chemistry(dt, 1, 1, 3)
    summary["timing_no_comm"] = e.comm_timing()
    assert summary["timing_no_comm"] == {"slabs": 0, "allreduce_ms": 0.0, "allreduce_exposed_ms": 0.0, "tail_ms": 0.0}
    e.close()
    e = engine(pkg, tables, heat16, [0, 0])
    try:
        e.comm_selftest(NSLAB)
        summary["multi_no_comm"] = "no error"
    except pkg.C2RayHipError as ex:
        summary["multi_no_comm"] = str(ex)
    assert "a multi-device context needs c2r_comm_init_local or c2r_comm_init first" in summary["multi_no_comm"]
    e.close()
    # 5. non-interference: three fused and three plain iterations with and without self-tests in between
    runs = []
    for selftests in (False, True):
        e = engine(pkg, tables, heat16, [0, 0])
        e.comm_init_local()
        runs.append(run_iterations(e, dt, 3, 3, selftests))
        e.close()
    for k in runs[0]:
        assert np.array_equal(runs[0][k], runs[1][k]), ("a self-test changed a later result", k)
    assert {f"{t}_{g}" for t in ("fused", "plain") for g in GRIDS} <= set(runs[0]), sorted(runs[0])
    np.savez(out / "honest_heat16_N2.npz", **runs[0])
    summary["non_interference_keys"] = sorted(runs[0])
    # 7. timings of the sum
    summary["timing"] = {}
    for n in (2, 4):
        e = engine(pkg, tables, heat16, [0] * n)
        e.comm_init_local()
        e.enable_timing(True)
        e.begin_step()
        rows = []
        for _ in range(2):
            e.set_rates_to_zero()
            t0 = time.perf_counter()
            e.pass_allreduce_chemistry(dt, 1, 1, 3)
            wall_ms = 1e3 * (time.perf_counter() - t0)
            for i in range(n):
                ct = e.comm_timing(i)
                rows.append({"wall_ms": wall_ms, **ct})
                print("comm timing", n, i, wall_ms, ct, flush=True)
                assert ct["slabs"] == min(3, (mesh[2] + 3) // 4), ct
                assert ct["tail_ms"] >= 0 and 0 <= ct["allreduce_exposed_ms"] <= ct["allreduce_ms"] < wall_ms, (ct, wall_ms)
        e.enable_timing(False)
        e.set_rates_to_zero()
        e.pass_allreduce_chemistry(dt, 1, 1, 3)
        off = [e.comm_timing(i) for i in range(n)]
        assert all(o == {"slabs": 0, "allreduce_ms": 0.0, "allreduce_exposed_ms": 0.0, "tail_ms": 0.0} for o in off), off
        summary["timing"][str(n)] = rows
        e.close()
    # 6. C2R_COMM_SELFTEST=1 with an honest library: both init calls succeed (and say so on stderr: the parent test reads it)
    os.environ["C2R_COMM_SELFTEST"] = "1"
    e = engine(pkg, tables, heat16, [0, 0])
    e.comm_init_local()
    assert e.rccl_ranks() == 2
    e.close()
    rep, err = threads_selftest(pkg, tables, heat16, 2)
    assert not any(err), err
    del os.environ["C2R_COMM_SELFTEST"]


def expected_bitflip_index(k, i, mesh, ncell):
    """position in the reduction buffer of element i of the k-th (1-based) all-reduce of a heating context's self-test"""
    if k == 1:
        return i
    slab, comp = divmod(k - 2, 4)
    if slab >= NSLAB:
        return 4 * ncell + i
    return comp * ncell + mesh[0] * mesh[1] * (mesh[2] * slab // NSLAB) + i


def mode_lie(pkg, tables, out, summary):
    lie = os.environ["FAKE_RCCL_CORRUPT"]
    heat16 = case_heating16(pkg)
    mesh = heat16[0]
    ncell = int(np.prod(mesh))
    library = pkg.HipEngine.comm_library()
    assert library.endswith("_fake_rccl_corrupt.so"), library
    summary.update(lie=lie, library=library, cases={})
    for n in (2, 4):
        e = engine(pkg, tables, heat16, [0] * n)
        e.comm_init_local()
        try:
            e.comm_selftest(NSLAB)
            raise AssertionError(f"the self-test passed over a transport that lies ({lie})")
        except pkg.C2RayHipError as ex:
            msg, rep = str(ex), ex.report
        print(lie, n, rep, msg, flush=True)
        assert rep["ranks"] == n and rep["devices"] == n and rep["elements"] == [4 * ncell + 48, 4 * ncell + 48], rep
        assert library in msg and "aborted" in msg, msg
        if lie.startswith("bitflip"):
            r, k, i = (int(x) for x in lie.split(":")[1:])
            index = expected_bitflip_index(k, i, mesh, ncell)
            assert sum(rep["mismatches"]) == 1 and rep["mismatches"][0 if k == 1 else 1] == 1, rep
            assert rep["bad_rank"] == r and rep["bad_index"] == index and rep["bad_route"] == (0 if k == 1 else 1), (rep, index)
            got, exp = (int(np.float64(x).view(np.uint64)) for x in (rep["got"], rep["expected"]))
            assert bin(got ^ exp).count("1") == 1, (hex(got), hex(exp))
            assert f"index {index} " in msg, msg
        elif lie == "fp32":
            assert rep["mismatches"] == [n * rep["elements"][0], n * rep["elements"][1]], rep
            assert rep["bad_route"] == 0 and rep["bad_rank"] == 0 and rep["bad_index"] == 0, rep
        else:
            r = int(lie.split(":")[1])
            assert rep["mismatches"] == rep["elements"], rep        # one device's worth: rank r's, nobody else's
            assert rep["bad_route"] == 0 and rep["bad_rank"] == r and rep["bad_index"] == 0, rep
        # the context refuses further collective work, at once
        t0 = time.time()
        try:
            e.allreduce_rates()
            again = "no error"
        except pkg.C2RayHipError as ex:
            again = str(ex)
        assert "was aborted after an earlier error" in again and time.time() - t0 < 5, again
        summary["cases"][str(n)] = dict(report=rep, message=msg, again=again)
        e.close()
    if lie != "fp32":
        return
    # 6. the switch makes the difference: with C2R_COMM_SELFTEST=1 the init calls fail with the self-test's text and leave no
    # communicator behind; without it the same lying library is accepted
    os.environ["C2R_COMM_SELFTEST"] = "1"
    e = engine(pkg, tables, heat16, [0, 0])
    try:
        e.comm_init_local()
        raise AssertionError("c2r_comm_init_local accepted a transport that lies")
    except pkg.C2RayHipError as ex:
        summary["init_local"] = str(ex)
    assert "c2r_comm_init_local (C2R_COMM_SELFTEST)" in summary["init_local"] and "WRONG" in summary["init_local"], summary["init_local"]
    assert e.comm_size() == 1 and e.rccl_ranks() == 0 and int(e.lib.c2r_comm_kind(e.h)) == 0
    e.close()
    _, err = threads_selftest(pkg, tables, heat16, 2)
    summary["init_rank"] = err
    assert all(x and "c2r_comm_init (C2R_COMM_SELFTEST)" in x and "WRONG" in x for x in err), err
    del os.environ["C2R_COMM_SELFTEST"]
    e = engine(pkg, tables, heat16, [0, 0])
    e.comm_init_local()
    assert e.rccl_ranks() == 2
    e.close()


def mode_transparent(pkg, tables, out, summary):
    """the lying library with nothing to lie about: the self-test passes and the iterations are the honest stand-in's"""
    assert not os.environ.get("FAKE_RCCL_CORRUPT")
    heat16 = case_heating16(pkg)
    summary["library"] = pkg.HipEngine.comm_library()
    assert summary["library"].endswith("_fake_rccl_corrupt.so")
    e = engine(pkg, tables, heat16, [0, 0])
    e.comm_init_local()
    check_ok(e.comm_selftest(NSLAB), 2, int(np.prod(heat16[0])), 4, 2)
    np.savez(out / "transparent_heat16_N2.npz", **run_iterations(e, heat16[5], 3, 0, False))
    e.close()


def exchange_id(pkg, out, rank):
    """rank 0 makes the id, the others read it from a file (what a launcher does by its own means)"""
    f = out / "unique_id.bin"
    if rank == 0:
        uid = pkg.HipEngine.comm_unique_id()
        (out / "unique_id.tmp").write_bytes(uid)
        (out / "unique_id.tmp").rename(f)
        return uid
    t0 = time.time()
    while not f.exists():
        assert time.time() - t0 < 60, "rank 0 did not publish the id"
        time.sleep(0.05)
    return f.read_bytes()


def mode_mp(pkg, tables, out, summary, rank, device):
    """one of two processes, a context each: fresh from create and with a heating set-up"""
    heat16 = case_heating16(pkg)
    ncell = int(np.prod(heat16[0]))
    e = engine(pkg, tables, heat16, device)
    e.comm_init(rank, 2, exchange_id(pkg, out, rank))
    rep = e.comm_selftest(NSLAB)
    check_ok(rep, 2, ncell, 4, 1)
    summary.update(report=rep, library=pkg.HipEngine.comm_library())
    e.begin_step()
    e.set_rates_to_zero()
    e.pass_allreduce_chemistry(heat16[5], 1 + rank, 2, 3)
    e.close()


def mode_gloo(pkg, tables, out, summary, rank, port):
    """RcclComm.selftest over two gloo ranks in two processes: what one rank saw, every rank raises"""
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=2)
    heat16 = case_heating16(pkg)
    e = engine(pkg, tables, heat16, 0)
    comm = pkg.parallel.RcclComm(e, dist)
    try:
        summary["report"] = comm.selftest(NSLAB)
        summary["error"] = None
    except RuntimeError as ex:
        summary["error"] = str(ex)
    dist.barrier()
    e.close()
    dist.destroy_process_group()


def mode_real_local(pkg, tables, out, summary):
    heat16 = case_heating16(pkg)
    e = engine(pkg, tables, heat16, [0, 1])
    e.comm_init_local()
    rep = e.comm_selftest(NSLAB)
    check_ok(rep, 2, int(np.prod(heat16[0])), 4, 2)
    summary.update(report=rep, library=pkg.HipEngine.comm_library())
    e.close()


def main():
    mode, out = sys.argv[1], Path(sys.argv[2])
    out.mkdir(parents=True, exist_ok=True)
    rank = int(sys.argv[3]) if len(sys.argv) > 3 else 0
    extra = int(sys.argv[4]) if len(sys.argv) > 4 else 0
    import __graft_entry__ as ge
    pkg = ge.load_package()
    tables = pkg.RadiationTables.load()
    summary = {}
    name = mode if mode not in ("mp", "gloo") else f"{mode}_rank{rank}"
    try:
        if mode in ("mp", "gloo"):
            globals()["mode_" + mode](pkg, tables, out, summary, rank, extra)
        else:
            globals()["mode_" + mode](pkg, tables, out, summary)
    finally:
        (out / f"{name}.json").write_text(json.dumps(summary, indent=1))
    print(f"comm_selftest_worker {name}: done", flush=True)


if __name__ == "__main__":
    main()
