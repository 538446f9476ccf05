#!/usr/bin/env python
"""Cost of the horizon loss (c2r_enable_horizon_loss) on bench.py's default workload: 256^3, 8 sources, isothermal, highly
ionised gas, one step = set_rates_to_zero + pass_sources + global_pass.  The settings alternate on one context in one process:
  off         the feature off, no horizons (bench.py's own pass)
  on          the feature on, no horizons: nothing may be launched, the times must be those of `off`
  off_r100    the feature off, every source a radius of 100 cells
  on_r100     the feature on, the same radii: k_horizon_rim and its finishing launch run inside the sweep's span, so the
              difference of sweep_ms to off_r100 is the added sweep-stream time
Every repeat is stored; the first round of settings is warm-up.  Times come from c2r_enable_timing (sweep, rates, chemistry
per step) and from the host clock around the steps.

    python tools/horizon_loss_cost.py [--mesh 256] [--sources 8] [--steps 10] [--repeats 4] [--radius 100] [--out FILE]
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
    ap.add_argument("--radius", type=float, default=100.0, help="cells")
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
    radii = [a.radius * float(grid.dr[0])] * a.sources
    settings = {"off": (False, None), "on": (True, None), "off_r100": (False, radii), "on_r100": (True, radii)}
    e.begin_step()

    def run(on, horizons):
        e.enable_horizon_loss(on)
        e.set_source_horizons(horizons)
        e.synchronize()
        acc = dict(step_ms=0.0, sweep_ms=0.0, rates_ms=0.0, chem_ms=0.0)
        launches = 0
        t0 = time.perf_counter()
        for _ in range(a.steps):
            e.set_rates_to_zero()
            e.pass_sources(1, 1)
            e.global_pass(dt)
            tm = e.timing()
            acc["sweep_ms"] += tm.sweep_ms
            acc["rates_ms"] += tm.rates_ms
            acc["chem_ms"] += tm.chem_ms
            launches = tm.sweep_launches
        e.synchronize()
        acc["step_ms"] = (time.perf_counter() - t0) * 1e3
        out = {k: v / a.steps for k, v in acc.items()}
        out["sweep_launches"] = launches
        out["photon_loss_1"] = float(e.get_loss()[0][0])
        if on:
            per, total = e.horizon_loss()
            out["horizon_loss_total"] = total
            out["horizon_loss_over_flux"] = [float(x) / (float(f) * src.S_star) for x, f in zip(per, src.NormFlux)]
        return out

    rows = {k: [] for k in settings}
    for _ in range(a.repeats + 1):
        for k, (on, horizons) in settings.items():
            rows[k].append(run(on, horizons))
    fields = ("step_ms", "sweep_ms", "rates_ms", "chem_ms")
    best = {k: {f: min(r[f] for r in v[1:]) for f in fields} for k, v in rows.items()}
    for k, v in rows.items():
        best[k]["sweep_launches"] = v[-1]["sweep_launches"]
    out = {"workload": f"config3 {a.mesh}^3 x {a.sources} sources, isothermal", "steps_per_repeat": a.steps,
           "radius_cells": a.radius, "best_of_repeats_after_the_first": best,
           "added_sweep_ms_on_r100_minus_off_r100": best["on_r100"]["sweep_ms"] - best["off_r100"]["sweep_ms"],
           "repeats": rows}
    print(json.dumps(out))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    e.close()


if __name__ == "__main__":
    main()
