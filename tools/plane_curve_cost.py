#!/usr/bin/env python
"""Cost of a plane with a light curve (c2r_set_plane_curve) against the same plane without one: one plane along z at N^3, z
open, x and y periodic, log-normal density, highly ionised gas, c2r_enable_timing on, c2r_do_source(NumSrc + 1) with NumSrc
= 0; isothermal and with heating.  Three variants alternate on one context in one process:
    uncurved   no curve: k_plane_rates and k_plane_exit
    ones       a two-step curve whose factors are all 1.0: k_pcurve_rates and k_pcurve_exit, the same work per cell
    far_dark   a three-step curve {1, 0.5, 2, 0} whose last step lies at two thirds of the depth: the far third is unlit
Every repeat is stored, the first is dropped from the best.  The figure compared is sweep_ms + rates_ms (the march; the
rates launch + the exit kernel + k_loss_finish).

    python tools/plane_curve_cost.py [--n 256] [--repeats 6] [--out FILE]
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
KINDS = ("uncurved", "ones", "far_dark")


def load(root):
    spec = importlib.util.spec_from_file_location("graft_entry_under_test", root / "__graft_entry__.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.load_package()


def curve_of(kind, n, d):
    depth = n * d
    if kind == "ones":
        return ([depth / 3.0, 2.0 * depth / 3.0], [1.0, 1.0, 1.0])
    if kind == "far_dark":
        return ([depth / 6.0, depth / 3.0, 2.0 * depth / 3.0], [1.0, 0.5, 2.0, 0.0])
    return None


def timing(pkg, n, repeats, heat):
    hp = pkg.hostphys
    mesh = (n, n, n)
    ncell = n ** 3
    rng = np.random.default_rng(1)
    ndens = hp.test_density(ZRED) * np.exp(rng.normal(0.0, 0.7, ncell))
    x = 1.0 - 10.0 ** rng.uniform(-4.5, -3.5, ncell)                       # ionised fraction: neutral 1e-4.5 .. 1e-3.5
    xh = np.concatenate([1.0 - x, x])
    xhe = np.concatenate([1.0 - x, 0.8 * x, 0.2 * x])
    temp = np.tile((1e4 * np.exp(rng.normal(0, 0.2, ncell))).astype(np.float32), 3) if heat else None
    (d, _, _), vol = hp.test_grid(n, ZRED)
    mat = pkg.Material(ndens, xh.copy(), xhe.copy(), temp, not heat, 1.0e4, 1.0, hp.reccoef(1.0e4))
    e = pkg.HipEngine(mesh, 0)
    e.set_boundaries((True, True, False))
    e.set_tables(pkg.RadiationTables.load())
    e.set_step(mat, pkg.GridProps(mesh, (d, d, d), vol), pkg.Cosmology(ZRED, hp.H0, hp.Omega0))
    e.set_sources(pkg.SourceProps(np.zeros((0, 3), dtype=np.int32), np.zeros(0), 1.0e48))
    e.upload_state(mat)
    e.enable_timing(True)
    e.set_plane_sources([(2, 0, FLUX)])
    runs = {k: [] for k in KINDS}
    for _ in range(repeats):
        for kind in KINDS:
            e.set_plane_curve(1, curve_of(kind, n, d))
            e.begin_step()
            e.upload_iter_state(xh, xhe)
            e.set_rates_to_zero()
            e.synchronize()
            t0 = time.perf_counter()
            e.do_source(1)
            wall = (time.perf_counter() - t0) * 1e3
            t = e.timing()
            runs[kind].append(dict(sweep_ms=t.sweep_ms, rates_ms=t.rates_ms, total_ms=t.sweep_ms + t.rates_ms, sweep_launches=t.sweep_launches,
                                   rates_launches=t.rates_launches, wall_ms=wall, plane_loss=e.plane_loss(1)))
    e.close()
    fields = ("sweep_ms", "rates_ms", "total_ms", "wall_ms")
    best = {k: {f: min(r[f] for r in v[1:]) for f in fields} for k, v in runs.items()}
    spread = {k: {f: max(r[f] for r in v[1:]) - min(r[f] for r in v[1:]) for f in fields[:3]} for k, v in runs.items()}
    return dict(best=best, spread=spread, all_repeats=runs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=6)
    ap.add_argument("--out", type=Path, default=None)
    a = ap.parse_args()
    pkg = load(Path(__file__).resolve().parent.parent)
    out = dict(n=a.n, repeats=a.repeats, kinds={k: str(curve_of(k, 3, 1.0)) + " in units of the depth / 3" for k in KINDS})
    for name, heat in (("isothermal", False), ("heating", True)):
        out[name] = timing(pkg, a.n, a.repeats, heat)
        print(json.dumps({name: dict(best=out[name]["best"], spread=out[name]["spread"])}), flush=True)
    if a.out:
        a.out.parent.mkdir(parents=True, exist_ok=True)
        a.out.write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    sys.exit(main())
