#!/usr/bin/env python
"""Cost of a plane with a flux map (c2r_set_plane_flux_map) against the same plane without one: one plane along z at N^3, z
open, x and y periodic, isothermal, log-normal density, highly ionised gas, c2r_enable_timing on, c2r_do_source(NumSrc + 1)
with NumSrc = 0.  The four kinds -- normal, tilted, normal with a map, tilted with a map -- alternate on one context in one
process; every repeat is stored, the first is dropped from the best.  sweep_ms is the march, rates_ms the rates launch +
the exit kernel + k_loss_finish.  The map is uniform (== normflux): the same work per cell as without it.

    python tools/plane_flux_map_cost.py [--n 128] [--repeats 6] [--root DIR] [--out FILE]
    python tools/plane_flux_map_cost.py --resources [--root DIR] [--out FILE]

--root: the checkout whose package is loaded (default: this one).  A checkout without c2r_set_plane_flux_map reports the
two kinds without a map only -- the parent commit's side of profiles/plane_flux_maps.json.
--resources: no GPU; the VGPR, SGPR, LDS and scratch figures of the plane kernels from the gfx950 code object in the library.
"""
import argparse
import importlib.util
import json
import re
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ZRED = 9.0
FLUX = 3.0e-41
TILT = (0.35, -0.6)
FIELDS = ("vgpr", "agpr", "sgpr", "lds", "scratch", "spill_v")  # the columns of tools/kernel_resources.py


def load(root):
    spec = importlib.util.spec_from_file_location("graft_entry_under_test", root / "__graft_entry__.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.load_package()


def resources(pkg):
    """{kernel name: {field: value}} of the plane kernels (k_plane_columns, k_plane_layer<FLUX>, k_plane_rates<HEAT, MULTI,
    FLUX>, k_plane_exit<MULTI, MAPPED, KEEP>; in a checkout from before they were merged also k_pflux_* and k_face_p*_exit),
    from the notes of the library's gfx950 code object (metadata only)."""
    sys.path.insert(0, str(Path(__file__).resolve().parent))
    import kernel_resources as kr
    rows = kr.resources(Path(pkg.build()))
    names = subprocess.run([kr.FILT], input="\n".join(r["name"] for r in rows), capture_output=True, text=True).stdout.splitlines()
    return {kr.short_name(nm): {f: int(r[f]) for f in FIELDS} for r, nm in zip(rows, names)
            if re.search(r"k_plane_|k_face_plane_exit|pflux", r["name"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=6)
    ap.add_argument("--root", type=Path, default=Path(__file__).resolve().parent.parent)
    ap.add_argument("--out", type=Path, default=None)
    ap.add_argument("--resources", action="store_true")
    a = ap.parse_args()
    pkg = load(a.root.resolve())
    if a.resources:
        out = resources(pkg)
        for k in sorted(out):
            print(k, out[k])
    else:
        out = timing(pkg, a)
    if a.out:
        a.out.parent.mkdir(parents=True, exist_ok=True)
        a.out.write_text(json.dumps(out, indent=1) + "\n")


def timing(pkg, a):
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
    has_map = hasattr(e, "set_plane_flux_map")
    fmap = np.zeros((3, n * n))
    fmap[0] = FLUX
    kinds = ["normal", "tilted"] + (["normal_map", "tilted_map"] if has_map else [])
    runs = {k: [] for k in kinds}
    for _ in range(a.repeats):
        for kind in kinds:
            e.set_plane_tilt(1, TILT if kind.startswith("tilted") else None)
            if has_map:
                e.set_plane_flux_map(1, fmap if kind.endswith("_map") else None)
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
    spread = {k: {f: max(r[f] for r in v[1:]) - min(r[f] for r in v[1:]) for f in ("sweep_ms", "rates_ms")} for k, v in runs.items()}
    print(json.dumps(dict(root=a.root.name, best=best, spread=spread)))
    return dict(n=n, tilt=TILT, root=a.root.name, best=best, spread=spread, all_repeats=runs)


if __name__ == "__main__":
    sys.exit(main())
