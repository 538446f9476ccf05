#!/usr/bin/env python3
"""First contact with a transport for the sum over ranks: verify it, then read one run.

    python tools/comm_firstcontact.py --gpus N [--mesh 256] [--steps 5] [--warmup 1] [--share-device]

One process drives N devices (c2r_create_multi + c2r_comm_init_local), the shape `bench.py --gpus N` takes by default; under
a launcher (WORLD_SIZE set) every rank runs this script with one device (c2r_create + c2r_comm_init over gloo, as bench.py
does).  It builds the bench's configs[2] workload (8 sources per device), makes the communicator, runs c2r_comm_selftest
FIRST -- a failed self-test ends the tool with status 2 before any step is timed -- then a warm-up and --steps fused
iterations with timing on, and prints ONE JSON line (rank 0): the self-test report; the library that carried the sums
(labelled STAND-IN, with rccl_ranks 0, unless its basename starts with librccl -- bench.py's rule); per device sweep_ms /
rates_ms / chem_ms and the comm timing (c2r_get_comm_timing), each with max, mean and max/mean over the devices; ms_per_step.
--share-device puts all N "devices" on GPU 0: a rehearsal, through a stand-in for RCCL when C2R_RCCL_LIBRARY names one
(tests/_fake_rccl.so), else through the library's in-process sum.  The tool starts no child process."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

KEYS = ("sweep_ms", "rates_ms", "chem_ms", "allreduce_ms", "allreduce_exposed_ms", "tail_ms")


def spread(rows, key):
    v = [r[key] for r in rows]
    mean = sum(v) / len(v)
    return {"max": max(v), "mean": mean, "max_over_mean": (max(v) / mean) if mean > 0 else None}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--gpus", type=int, required=True)
    ap.add_argument("--mesh", type=int, default=256)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--share-device", action="store_true")
    a = ap.parse_args()
    if a.share_device and os.environ.get("C2R_RCCL_LIBRARY"):
        os.environ.setdefault("C2R_COMM_SHARED_DEVICE_RCCL", "1")   # a stand-in accepts devices that repeat; RCCL does not

    import bench                     # the input builders only; nothing of it is edited or run
    import torch
    pkg = bench.ge.load_package()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    launched = world > 1
    rank = int(os.environ.get("RANK", "0")) if launched else 0
    if launched and a.gpus != world:
        raise SystemExit(f"comm_firstcontact.py --gpus {a.gpus} inside a launch of WORLD_SIZE={world}")
    if launched:
        local = 0 if a.share_device else int(os.environ.get("LOCAL_RANK", "0"))
        devices = local
    else:
        have = torch.cuda.device_count()
        if have < a.gpus and not a.share_device:
            raise SystemExit(f"comm_firstcontact.py --gpus {a.gpus}: only {have} HIP device(s) visible (--share-device rehearses on one)")
        devices = [0] * a.gpus if a.share_device else list(range(a.gpus))
    n = a.mesh
    mat, grid, src, cosmo = bench.config3_inputs(pkg, n, 8 * a.gpus)
    e = pkg.HipEngine((n, n, n), devices)
    e.set_tables(pkg.RadiationTables.load())
    e.set_step(mat, grid, cosmo)
    e.set_sources(src)
    e.upload_state(mat)
    e.set_batch(8)
    e.enable_timing(True)
    nslab = int(os.environ.get("C2R_ALLREDUCE_SLABS", "4"))
    dist = None
    try:
        if launched:
            import torch.distributed as dist
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", "29511")
            dist.init_process_group("gloo", rank=rank, world_size=world)   # plumbing only: the RCCL id and the agreements
            comm = pkg.parallel.RcclComm(e, dist)
        else:
            e.comm_init_local()
            comm = pkg.parallel.LocalComm(e)
        report = comm.selftest(nslab)                                       # before anything is timed
    except Exception as ex:  # noqa: BLE001 -- whatever the library reports
        out = {"tool": "comm_firstcontact", "ok": False, "error": str(ex), "selftest": getattr(ex, "report", None)}
        if rank == 0:
            print(json.dumps(out), flush=True)
        sys.stderr.write(f"comm_firstcontact.py: rank {rank}: {ex}\n")
        return 2
    kind = report["kind"]
    rccl_ranks = e.rccl_ranks()
    library = pkg.HipEngine.comm_library() if kind == 1 else None
    if kind != 1:
        label = "in-process sum of replicas that share a device (rehearsal): no RCCL"
    elif os.path.basename(library).startswith("librccl"):
        label = f"RCCL ({library})"
    else:
        label = f"STAND-IN for RCCL ({library}, C2R_RCCL_LIBRARY) -- NOT an RCCL result"
        rccl_ranks = 0

    dt = 1.0e7 * pkg.hostphys.YEAR
    e.begin_step()

    def step():
        e.set_rates_to_zero()
        return comm.pass_allreduce_chemistry(e, dt, nslab)

    def barrier():
        e.synchronize()
        if dist is not None:
            dist.barrier()

    for _ in range(a.warmup):
        step()
    barrier()
    ndev = e.num_devices()
    rows = [dict.fromkeys(KEYS, 0.0) for _ in range(ndev)]
    slabs = [0] * ndev
    t0 = time.perf_counter()
    for _ in range(a.steps):
        step()
        for i, row in enumerate(rows):
            tm, ct = e.timing(i), e.comm_timing(i)
            for k in ("sweep_ms", "rates_ms", "chem_ms"):
                row[k] += getattr(tm, k)
            for k in ("allreduce_ms", "allreduce_exposed_ms", "tail_ms"):
                row[k] += ct[k]
            slabs[i] = ct["slabs"]
    barrier()
    elapsed = time.perf_counter() - t0
    steps = max(a.steps, 1)
    rows = [{"slabs": slabs[i], **{k: v / steps for k, v in row.items()}} for i, row in enumerate(rows)]
    mine = {"elapsed": elapsed, "devices": rows, "selftest": report}
    if launched:
        allr = [None] * world
        dist.all_gather_object(allr, mine)
    else:
        allr = [mine]
    if rank == 0:
        devs = [r for m in allr for r in m["devices"]]
        out = {"tool": "comm_firstcontact", "ok": True, "gpus": a.gpus, "mesh": n, "steps": a.steps, "warmup": a.warmup, "nslab": nslab,
               "shape": "one rank per device (launcher)" if launched else "one process, all devices",
               "share_device": bool(a.share_device), "transport": label, "library": library, "rccl_ranks": rccl_ranks,
               "selftest": report, "selftest_other_ranks": [m["selftest"] for m in allr[1:]],
               "devices": devs, "over_devices": {k: spread(devs, k) for k in KEYS},
               "ms_per_step": 1e3 * max(m["elapsed"] for m in allr) / steps}
        print(json.dumps(out), flush=True)
    e.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
