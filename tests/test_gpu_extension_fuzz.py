"""Seeded fuzz of the extensions on the GPU against the one composer of tests/extension_fuzz_cases.py: open and per-axis
boundaries, escape maps, planes (normal, tilted, flux-mapped), beams, photon horizons and the horizon loss, several of them in
one pass, on meshes with axes of 2, 3 or 5 cells, cells that are no cubes, radii exactly on a lattice distance, cos_half of
0, 1 and sqrt(1/2), sources that share a cell.  tests/test_extension_fuzz_host.py proves on the CPU that every case of the
list is well-posed.   python -m pytest tests -m gpu.   C2R_EXTFUZZ_CASES / C2R_EXTFUZZ_SEED widen or move the list.

One case is one test id.  The bar is np.array_equal with the printed spec as the tag: phih_grid, phihe_grid, phiheat, sum_nbox,
the rounds and the final box of every source, every open face's escape map and total, each plane's exit columns and exit
flux, the horizon loss per source == rim_reference.face_sum of the expected terms and their total, the rim terms of the
horizoned source swept last, and after the global pass the non-converged count, the four iteration-state arrays and the
temperature.  Two sums that the device adds in another order than their reference keep the bounds the project already has
for them (tests/test_gpu_plane_mix.py): c2r_get_plane_loss 1e-13 relative against math.fsum of the plane's terms, and
photon_loss(1) 1e-12 relative where mix_reference.has_loss_reference holds and no beam or horizon is set.
Measured on one MI355X: the 28 ids of the default list take 4.6 s, references included; the first id, which also starts the
GPU runtime, 0.38 s, the slowest after it (several rounds on the 11 x 24 x 24 mesh) 0.33 s, the median 0.14 s -- beside 0.19 s
for the slowest id of tests/test_gpu_horizon_loss.py in the same run.  Most of an id is the oracle on the CPU.
"""
import numpy as np
import pytest

import extension_fuzz_cases as xf
import mix_reference as mr
import rim_reference as rr
from conftest import rel_err
from test_gpu_fuzz import _progress  # a line per case in the progress log that file keeps
from test_gpu_plane_mix import make_engine, otables3, tables3  # noqa: F401  (fixtures: both sets of tables with three SEDs)

pytestmark = pytest.mark.gpu
SPECS = xf.case_list()


def run_route(e, cfg, nsrc):
    """The drawn route from zeroed rates, right after begin_step.  Returns the non-converged count where the route ran the
    global pass itself, else None."""
    e.begin_step()
    e.set_rates_to_zero()
    route = cfg["route"]
    if route == "plain":
        e.pass_sources(1, 1)
    elif route == "slabs":
        for s in range(e.pass_sources_begin(1, 1, cfg["nslab"])):
            e.pass_wait_slab(s)
        e.pass_sources_end()
    elif route == "iteration":
        return e.iteration(cfg["dt"], 1, 1, cfg["nslab"])["conv_flag"]
    elif route == "do_source":                              # the planes first, as a pass runs them, then source by source
        for p in range(1, len(cfg["planes"]) + 1):
            e.do_source(nsrc + p)
        for ns in range(1, nsrc + 1):
            e.do_source(ns)
    else:
        raise ValueError(route)
    return None


@pytest.mark.parametrize("ic", range(len(SPECS)))
def test_case_against_the_composition(pkg, orc, otables3, tables3, ic):
    spec = SPECS[ic]
    tag = xf.tag(ic, spec)
    _progress(tag)
    print(tag)
    case, cfg = xf.build(pkg, spec)
    mix = xf.compose_all(pkg, orc, otables3, case, spec)
    assert all(mix["same_cells"]), (mix["oracle_nbox"], tag)
    nsrc, planes = len(case.flux), cfg["planes"]
    e = make_engine(pkg, tables3, case, planes, maps=cfg["maps"], batch=cfg["batch"])
    if cfg["horizon_loss"]:
        e.enable_horizon_loss()
    e.set_source_horizons(cfg["horizons"])
    e.set_source_beams(cfg["beams"])
    conv = run_route(e, cfg, nsrc)
    got = e.download_rates()
    # the rounds and the boxes first: everything below supposes them
    traces = [e.source_trace(ns) for ns in range(1, nsrc + 1)]
    print("rounds", [t["nbox"] for t in traces], "expected", [t[0] for t in mix["trace"]], "unbeamed", mix["oracle_nbox"])
    for ns, (tr, (nbox, lo, hi)) in enumerate(zip(traces, mix["trace"]), start=1):
        assert (tr["nbox"], tr["box_lo"], tr["box_hi"]) == (nbox, lo, hi), (ns, tr, tag)
    assert got["sum_nbox"] == mix["sum_nbox"], (got["sum_nbox"], mix["sum_nbox"], tag)
    # the rate grids
    for k in ("phih_grid", "phihe_grid") + (("phiheat",) if case.heat else ()):
        bad = int(np.count_nonzero(got[k] != mix[k]))
        print(k, "cells", got[k].size, "non-zero", int(np.count_nonzero(mix[k])), "differ", bad, "worst rel", float(np.max(rel_err(got[k], mix[k]))))
        assert np.array_equal(got[k], mix[k]), (k, bad, tag)
    if not case.heat:
        assert not got["phiheat"].any(), tag
    # the escape maps and their totals
    if cfg["maps"]:
        totals = e.face_loss()
        for f in range(6):
            if f not in mix["maps"]:
                assert totals[f] == 0.0, (f, tag)
                continue
            have, want = e.face_loss_map(f), mix["maps"][f]
            bad = int(np.count_nonzero(have != want)) if have.shape == want.shape else -1
            print("face", f, "cells", want.size, "non-zero", int(np.count_nonzero(want)), "differ", bad, "total", totals[f])
            assert have.shape == want.shape and np.array_equal(have, want), (f, bad, tag)
            assert totals[f] == rr.face_sum(want.reshape(-1)), (f, tag)
    # the planes
    for p, ref in mix["plane"].items():
        assert np.array_equal(e.plane_exit_columns(p), ref["exit"]), (p, tag)
        if mr.plane_kind(planes[p - 1])[1]:
            assert np.array_equal(e.plane_exit_flux(p), ref["exit_flux"]), (p, tag)
        loss = e.plane_loss(p)
        print("plane", p, "loss", loss, "reference", ref["loss"], "rel", rel_err(loss, ref["loss"]) if ref["loss"] > 0 else 0.0)
        assert rel_err(loss, ref["loss"]) <= 1e-13 if ref["loss"] > 0 else loss == 0.0, (p, tag)
    # the horizon loss
    if cfg["horizon_loss"]:
        per, total = e.horizon_loss()
        print("horizon loss", per, "expected", mix["horizon_loss"])
        assert np.array_equal(per, mix["horizon_loss"]), tag
        assert total == mix["horizon_total"], tag
        if mix["rim_source"] is not None:
            ns = mix["rim_source"]
            got_ns, got_ext, terms = e.horizon_rim()
            _, lo, hi = mix["trace"][ns - 1]
            want = mix["horizon_terms"][ns]
            bad = int(np.count_nonzero(terms != want)) if terms.shape == want.shape else -1
            print("rim of source", got_ns, "extents", got_ext, "terms", terms.size, "faces", int(np.count_nonzero(want)), "differ", bad)
            assert got_ns == ns and got_ext == rr.extents(lo, hi), tag
            assert np.array_equal(terms, want) and not np.signbit(terms).any(), (bad, tag)
    # photon_loss(1), where it has a reference
    assert not got["photon_loss"][1:].any(), tag
    if mix["loss"] is not None:
        loss = got["photon_loss"][0]
        print("photon_loss(1)", loss, "reference", mix["loss"], "rel", rel_err(loss, mix["loss"]) if mix["loss"] > 0 else 0.0)
        assert rel_err(loss, mix["loss"]) <= 1e-12 if mix["loss"] > 0 else loss == 0.0, tag
    # the global pass
    if conv is None:
        conv = e.global_pass(cfg["dt"])
    assert conv == mix["conv"], (conv, mix["conv"], tag)
    it = e.download_iter_state()
    for k in ("xh_av", "xhe_av", "xh_intermed", "xhe_intermed"):
        assert np.array_equal(it[k], mix[k]), (k, tag)
    if case.heat:
        ncell = got["phih_grid"].size
        mat = pkg.Material(None, np.empty(2 * ncell), np.empty(3 * ncell), np.empty(3 * ncell, dtype=np.float32), False)
        e.download_state(mat)
        assert np.array_equal(mat.temperature_grid, mix["temperature"]), tag
    e.close()
    _progress(f"case {ic} done")
