#!/usr/bin/env python
"""Cost of a point source outside the mesh (c2r_set_sources_external): bench.py's gas (256^3, isothermal, highly ionised, so
the source runs to its reach), OPEN boundaries, one source in the middle of the +z face -- on the face cell (c2r_set_sources),
and 1, 32 and 128 cells beyond the face.  One step = set_rates_to_zero + pass_sources; sweep_ms and rates_ms from
c2r_enable_timing, the cells of the box (vacuum included) and the entries of the column block from c2r_get_source_trace.  The
settings alternate on one context; every repeat is stored, the first round of settings is warm-up.

    python tools/external_source_cost.py [--mesh 256] [--steps 3] [--repeats 3] [--out FILE]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", type=int, default=256)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import __graft_entry__ as ge
    import bench
    pkg = ge.load_package()
    n = a.mesh
    mat, grid, src, cosmo = bench.config3_inputs(pkg, n, 1)
    e = pkg.HipEngine((n,) * 3, 0)
    e.set_boundaries(False)
    e.set_tables(pkg.RadiationTables.load())
    e.set_step(mat, grid, cosmo)
    e.upload_state(mat)
    e.enable_timing(True)
    e.begin_step()
    flux = np.asarray(src.NormFlux, dtype=np.float64)[:1]

    def run(dist):
        s = pkg.SourceProps(np.array([[n // 2, n // 2, n + dist]], dtype=np.int32), flux, src.S_star)
        if dist == 0:
            e.set_sources(s)
        else:
            e.set_sources_external(s)
        e.synchronize()
        acc = dict(step_ms=0.0, sweep_ms=0.0, rates_ms=0.0)
        t0 = time.perf_counter()
        for _ in range(a.steps):
            e.set_rates_to_zero()
            e.pass_sources(1, 1)
            tm = e.timing()
            acc["sweep_ms"] += tm.sweep_ms
            acc["rates_ms"] += tm.rates_ms
        e.synchronize()
        acc["step_ms"] = (time.perf_counter() - t0) * 1e3
        out = {k: v / a.steps for k, v in acc.items()}
        t = e.source_trace(1)
        out.update(sum_nbox=e.get_loss()[1], swept_cells=t["swept_cells"], block_cells=t["block_cells"], sweep_threads=t["sweep_threads"])
        return out

    settings = {"on_the_face": 0, "beyond_1": 1, "beyond_32": 32, "beyond_128": 128}
    rows = {k: [] for k in settings}
    for _ in range(a.repeats + 1):
        for k, dist in settings.items():
            rows[k].append(run(dist))
    best = {k: {f: min(r[f] for r in v[1:]) for f in ("step_ms", "sweep_ms", "rates_ms")} for k, v in rows.items()}
    for k, v in rows.items():
        for f in ("sum_nbox", "swept_cells", "block_cells", "sweep_threads"):
            best[k][f] = v[-1][f]
    out = {"workload": f"{n}^3, open boundaries, one source in the middle of the +z face and beyond it, isothermal, ionised gas",
           "steps_per_repeat": a.steps, "best_of_repeats_after_the_first": best, "repeats": rows}
    print(json.dumps(out))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    e.close()


if __name__ == "__main__":
    main()
