#!/usr/bin/env python
"""Cost of beamed point sources (c2r_set_source_beams) on bench.py's default workload: 256^3, 8 sources, isothermal, highly
ionised gas, one step = set_rates_to_zero + pass_sources + global_pass.  Two settings alternate on one context in one
process: no beams (the rates launches are k_rates) and all eight sources beamed as cones of a given half angle about
different axes (the launches are k_rates_beam; unlit lanes skip their band loops, a wave retires early only when all 64
lanes of its 4 x 4 x 4 cube are unlit).  Every repeat is stored; the first pair is warm-up.  Times come from
c2r_enable_timing (sweep, rates, chemistry per step) and from the host clock around the steps.

    python tools/source_beams_cost.py [--mesh 256] [--sources 8] [--steps 10] [--repeats 4] [--half-angle 30] [--out FILE]
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
    ap.add_argument("--sources", type=int, default=8)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--half-angle", type=float, default=30.0)
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
    rng = np.random.default_rng(30)
    cos_half = float(np.cos(np.radians(a.half_angle)))
    cones = [(1, tuple(float(x) for x in rng.normal(size=3)), cos_half) for _ in range(a.sources)]
    e.begin_step()

    def run(beams):
        e.set_source_beams(beams)
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

    rows = {"unbeamed": [], "beamed": []}
    for _ in range(a.repeats + 1):
        rows["unbeamed"].append(run(None))
        rows["beamed"].append(run(cones))
    best = {k: {f: min(r[f] for r in v[1:]) for f in ("step_ms", "sweep_ms", "rates_ms", "chem_ms")} for k, v in rows.items()}
    out = {"workload": f"config3 {a.mesh}^3 x {a.sources} sources, isothermal", "half_angle_deg": a.half_angle, "steps_per_repeat": a.steps,
           "best_of_repeats_after_the_first": best, "repeats": rows}
    line = json.dumps(out)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    e.close()


if __name__ == "__main__":
    main()
