#!/usr/bin/env python
"""Cost of photon horizons (c2r_set_source_horizons) on bench.py's default workload: 256^3, 8 sources, isothermal, highly
ionised gas, one step = set_rates_to_zero + pass_sources + global_pass.  The settings alternate on one context in one process:
  none        no horizons set (the rates launches are k_rates)
  bicone      no horizons, every source a bicone with cos_half = 0: every cell lit through k_rates_beam, the beam's predicate alone
  huge        every source radius = 1e200 (R2 = +inf): every cell lit through k_rates_beam, the horizon's predicate alone
  r80, r40    every source a radius of 80 and of 40 cells (the sub-box loop ends at the first box that holds the sphere)
Every repeat is stored; the first round of settings is warm-up.  Times come from c2r_enable_timing (sweep, rates, chemistry per
step) and from the host clock around the steps; cells_swept and rounds from c2r_get_source_trace, summed over the sources.

    python tools/source_horizon_cost.py [--mesh 256] [--sources 8] [--steps 10] [--repeats 4] [--out FILE]
"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", type=int, default=256)
    ap.add_argument("--sources", type=int, default=8)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import __graft_entry__ as ge
    import bench
    pkg = ge.load_package()
    mat, grid, src, cosmo = bench.config3_inputs(pkg, a.mesh, a.sources)
    e = pkg.HipEngine((a.mesh,) * 3, 0)
    e.set_tables(pkg.RadiationTables.load())
    e.set_step(mat, grid, cosmo)
    e.set_sources(src)
    e.upload_state(mat)
    e.set_batch(8)
    e.enable_timing(True)
    dt = 1.0e7 * pkg.hostphys.YEAR
    dr = float(grid.dr[0])
    full = [(2, (0.0, 0.0, 1.0), 0.0)] * a.sources
    settings = {"none": (None, None), "bicone": (full, None), "huge": (None, [1e200] * a.sources),
                "r80": (None, [80.0 * dr] * a.sources), "r40": (None, [40.0 * dr] * a.sources)}
    e.begin_step()

    def run(beams, horizons):
        e.set_source_beams(beams)
        e.set_source_horizons(horizons)
        e.synchronize()
        acc = dict(step_ms=0.0, sweep_ms=0.0, rates_ms=0.0, chem_ms=0.0)
        t0 = time.perf_counter()
        for _ in range(a.steps):
            e.set_rates_to_zero()
            e.pass_sources(1, 1)
            e.global_pass(dt)
            tm = e.timing()
            acc["sweep_ms"] += tm.sweep_ms
            acc["rates_ms"] += tm.rates_ms
            acc["chem_ms"] += tm.chem_ms
        e.synchronize()
        acc["step_ms"] = (time.perf_counter() - t0) * 1e3
        out = {k: v / a.steps for k, v in acc.items()}
        out["sum_nbox"] = e.get_loss()[1]
        out["cells_swept"] = sum(e.source_trace(ns)["swept_cells"] for ns in range(1, a.sources + 1))
        return out

    rows = {k: [] for k in settings}
    for _ in range(a.repeats + 1):
        for k, (beams, horizons) in settings.items():
            rows[k].append(run(beams, horizons))
    best = {k: {f: min(r[f] for r in v[1:]) for f in ("step_ms", "sweep_ms", "rates_ms", "chem_ms")} for k, v in rows.items()}
    for k, v in rows.items():
        best[k]["sum_nbox"], best[k]["cells_swept"] = v[-1]["sum_nbox"], v[-1]["cells_swept"]
    out = {"workload": f"config3 {a.mesh}^3 x {a.sources} sources, isothermal", "steps_per_repeat": a.steps,
           "best_of_repeats_after_the_first": best, "repeats": rows}
    print(json.dumps(out))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    e.close()


if __name__ == "__main__":
    main()
