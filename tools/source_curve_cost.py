#!/usr/bin/env python
"""Cost of source light curves (c2r_set_source_curves) on bench.py's default workload: 256^3, 8 sources, isothermal, highly
ionised gas, one step = set_rates_to_zero + pass_sources + global_pass.  The settings alternate on one context in one process:
  none        nothing set (the rates launches are k_rates)
  huge        every source a horizon of radius 1e200 (R2 = +inf): every cell lit through k_rates_beam
  curve1      every source a one-step curve, radius 40 cells, factors 1.0: the bare bits through k_rates_curve
  curve8      every source an eight-step curve, radii 10, 20, ... 80 cells, factors 1.0
Every factor is 1.0, so all four settings compute the same grids in the same rounds and differ only in the rates kernel.
Every repeat is stored; the first round of settings is warm-up.  Times come from c2r_enable_timing (sweep, rates, chemistry per
step) and from the host clock around the steps.  The report compares rates_ms of the two curve settings with `huge`, the
k_rates_beam setting of the same job, beside the spread of that setting's own repeats.

    python tools/source_curve_cost.py [--mesh 256] [--sources 8] [--steps 10] [--repeats 4] [--out FILE]
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
    one = ([40.0 * dr], [1.0, 1.0])
    eight = ([10.0 * (k + 1) * dr for k in range(8)], [1.0] * 9)
    settings = {"none": (None, None), "huge": ([1e200] * a.sources, None), "curve1": (None, [one] * a.sources),
                "curve8": (None, [eight] * a.sources)}
    e.begin_step()

    def run(horizons, curves):
        e.set_source_horizons(horizons)
        e.set_source_curves(curves)
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
        return out

    rows = {k: [] for k in settings}
    for _ in range(a.repeats + 1):
        for k, (horizons, curves) in settings.items():
            rows[k].append(run(horizons, curves))
    fields = ("step_ms", "sweep_ms", "rates_ms", "chem_ms")
    best = {k: {f: min(r[f] for r in v[1:]) for f in fields} for k, v in rows.items()}
    spread = {k: {f: max(r[f] for r in v[1:]) - min(r[f] for r in v[1:]) for f in fields} for k, v in rows.items()}
    for k, v in rows.items():
        best[k]["sum_nbox"] = v[-1]["sum_nbox"]
    against = {k: {"rates_ms_best": best[k]["rates_ms"], "k_rates_beam_rates_ms_best": best["huge"]["rates_ms"],
                   "ratio": best[k]["rates_ms"] / best["huge"]["rates_ms"],
                   "k_rates_beam_spread_over_its_repeats_ms": spread["huge"]["rates_ms"]} for k in ("curve1", "curve8")}
    out = {"workload": f"config3 {a.mesh}^3 x {a.sources} sources, isothermal", "steps_per_repeat": a.steps,
           "recipe": "python tools/source_curve_cost.py --out profiles/source_curves.json",
           "curves_against_k_rates_beam": against, "best_of_repeats_after_the_first": best,
           "spread_of_repeats_after_the_first": spread, "repeats": rows}
    print(json.dumps({k: out[k] for k in ("workload", "curves_against_k_rates_beam", "best_of_repeats_after_the_first")}))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    e.close()


if __name__ == "__main__":
    main()
