#!/usr/bin/env python
"""Cost of the column march of a tilted plane (one k_plane_layer launch per layer) against an untilted one
(k_plane_columns): one plane along z at N^3, z open, x and y periodic, isothermal, log-normal density, highly ionised gas,
c2r_enable_timing on, c2r_do_source(NumSrc + 1) with NumSrc = 0.  Untilted and tilted alternate on one context in one
process; the first repeat is dropped, the best of the rest is reported.  sweep_ms is the march, rates_ms is k_plane_rates +
k_plane_exit + k_loss_finish.

    python tools/oblique_plane_cost.py [--n 256] [--repeats 5] [--root DIR] [--out FILE]

--root: the checkout whose package is loaded (default: this one).  A checkout without c2r_set_plane_tilt reports the
untilted figure only -- the parent commit's side of profiles/oblique_planes.json.
"""
import argparse
import importlib.util
import json
import sys
import time
from pathlib import Path

import numpy as np

ZRED = 9.0
FLUX = 3.0e-41
TILT = (0.35, -0.6)


def load(root):
    spec = importlib.util.spec_from_file_location("graft_entry_under_test", root / "__graft_entry__.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.load_package()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--root", type=Path, default=Path(__file__).resolve().parent.parent)
    ap.add_argument("--out", type=Path, default=None)
    a = ap.parse_args()
    pkg = load(a.root.resolve())
    hp = pkg.hostphys
    n = a.n
    mesh = (n, n, n)
    ncell = n ** 3
    rng = np.random.default_rng(1)
    ndens = hp.test_density(ZRED) * np.exp(rng.normal(0.0, 0.7, ncell))
    x = 1.0 - 10.0 ** rng.uniform(-4.5, -3.5, ncell)                       # ionised fraction: neutral 1e-4.5 .. 1e-3.5
    xh = np.concatenate([1.0 - x, x])
    xhe = np.concatenate([1.0 - x, 0.8 * x, 0.2 * x])
    (d, _, _), vol = hp.test_grid(n, ZRED)
    mat = pkg.Material(ndens, xh.copy(), xhe.copy(), None, True, 1.0e4, 1.0, hp.reccoef(1.0e4))
    e = pkg.HipEngine(mesh, 0)
    e.set_boundaries((True, True, False))
    e.set_tables(pkg.RadiationTables.load())
    e.set_step(mat, pkg.GridProps(mesh, (d, d, d), vol), pkg.Cosmology(ZRED, hp.H0, hp.Omega0))
    e.set_sources(pkg.SourceProps(np.zeros((0, 3), dtype=np.int32), np.zeros(0), 1.0e48))
    e.upload_state(mat)
    e.enable_timing(True)
    e.set_plane_sources([(2, 0, FLUX)])
    has_tilt = hasattr(e, "set_plane_tilt")
    kinds = ["untilted", "tilted"] if has_tilt else ["untilted"]
    runs = {k: [] for k in kinds}
    for _ in range(a.repeats):
        for kind in kinds:
            if has_tilt:
                e.set_plane_tilt(1, TILT if kind == "tilted" else None)
            e.begin_step()
            e.upload_iter_state(xh, xhe)
            e.set_rates_to_zero()
            e.synchronize()
            t0 = time.perf_counter()
            e.do_source(1)
            wall = (time.perf_counter() - t0) * 1e3
            t = e.timing()
            runs[kind].append(dict(sweep_ms=t.sweep_ms, rates_ms=t.rates_ms, sweep_launches=t.sweep_launches,
                                   rates_launches=t.rates_launches, wall_ms=wall, plane_loss=e.plane_loss(1)))
    e.close()
    best = {k: {f: min(r[f] for r in v[1:]) for f in ("sweep_ms", "rates_ms", "wall_ms")} for k, v in runs.items()}
    for k, v in runs.items():
        best[k]["sweep_launches"] = v[-1]["sweep_launches"]
    out = dict(n=n, tilt=TILT if has_tilt else None, root=a.root.name, best=best, all_repeats=runs)
    if has_tilt:
        out["tilted_over_untilted_sweep"] = best["tilted"]["sweep_ms"] / best["untilted"]["sweep_ms"]
    text = json.dumps(out, indent=1)
    print(json.dumps(dict(best=best, ratio=out.get("tilted_over_untilted_sweep"))))
    if a.out:
        a.out.parent.mkdir(parents=True, exist_ok=True)
        a.out.write_text(text + "\n")


if __name__ == "__main__":
    sys.exit(main())
