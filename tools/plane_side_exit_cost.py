#!/usr/bin/env python
"""Cost of the side exit of a tilted plane (c2r_enable_plane_side_exit): one plane along z at N^3 with a flux map, all axes
open, isothermal, log-normal density, highly ionised gas, c2r_enable_timing on, c2r_do_source(NumSrc + 1) with NumSrc = 0.
Side exit off and on alternate on one context in one process; every repeat is stored, the first is dropped.  sweep_ms is the
march: N launches of k_plane_layer<true> (off) or k_pside_layer<true> (on, both sides live).

    python tools/plane_side_exit_cost.py [--n 128] [--repeats 6] [--out FILE]
"""
import argparse
import importlib.util
import json
import sys
from pathlib import Path

import numpy as np

ZRED = 9.0
FLUX = 3.0e-41
TILT = (0.35, -0.6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=6)
    ap.add_argument("--out", type=Path, default=None)
    a = ap.parse_args()
    root = Path(__file__).resolve().parent.parent
    spec = importlib.util.spec_from_file_location("graft_entry_under_test", root / "__graft_entry__.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    pkg = mod.load_package()
    hp = pkg.hostphys
    n = a.n
    mesh = (n, n, n)
    rng = np.random.default_rng(1)
    ndens = hp.test_density(ZRED) * np.exp(rng.normal(0.0, 0.7, n ** 3))
    x = 1.0 - 10.0 ** rng.uniform(-4.5, -3.5, n ** 3)
    xh = np.concatenate([1.0 - x, x])
    xhe = np.concatenate([1.0 - x, 0.8 * x, 0.2 * x])
    (d, _, _), vol = hp.test_grid(n, ZRED)
    mat = pkg.Material(ndens, xh.copy(), xhe.copy(), None, True, 1.0e4, 1.0, hp.reccoef(1.0e4))
    e = pkg.HipEngine(mesh, 0)
    e.set_boundaries((False, False, False))
    e.set_tables(pkg.RadiationTables.load())
    e.set_step(mat, pkg.GridProps(mesh, (d, d, d), vol), pkg.Cosmology(ZRED, hp.H0, hp.Omega0))
    e.set_sources(pkg.SourceProps(np.zeros((0, 3), dtype=np.int32), np.zeros(0), 1.0e48))
    e.upload_state(mat)
    e.enable_timing(True)
    e.set_plane_sources([(2, 0, FLUX)])
    e.set_plane_tilt(1, TILT)
    fmap = np.zeros((3, n * n))
    fmap[0] = FLUX
    e.set_plane_flux_map(1, fmap)
    runs = {"off": [], "on": []}
    for _ in range(a.repeats):
        for kind in runs:
            e.enable_plane_side_exit(1, kind == "on")
            e.begin_step()
            e.upload_iter_state(xh, xhe)
            e.set_rates_to_zero()
            e.synchronize()
            e.do_source(1)
            t = e.timing()
            runs[kind].append(dict(sweep_ms=t.sweep_ms, rates_ms=t.rates_ms, sweep_launches=t.sweep_launches))
    e.close()
    out = dict(n=n, tilt=TILT, sweep_ms={k: [r["sweep_ms"] for r in v[1:]] for k, v in runs.items()}, all_repeats=runs)
    print(json.dumps(dict(n=n, sweep_ms=out["sweep_ms"])))
    if a.out:
        a.out.parent.mkdir(parents=True, exist_ok=True)
        a.out.write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    sys.exit(main())
