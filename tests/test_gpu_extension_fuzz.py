"""Seeded fuzz of the extensions on the GPU against the one composer of tests/extension_fuzz_cases.py: open and per-axis
boundaries, escape maps, planes (normal, tilted, flux-mapped), beams, photon horizons and the horizon loss, several of them in
one pass, on meshes with axes of 2, 3 or 5 cells, cells that are no cubes, radii exactly on a lattice distance, cos_half of
0, 1 and sqrt(1/2), sources that share a cell.  Behind the default list comes the curved list: the same draws with a source
light curve per point source (c2r_set_source_curves: none, factors of 0 and 1 only, all ones, the horizon-equal step, a dark
gap, eight steps; radii uniform, on a lattice distance and one ulp either side, below a cell, 0 and 1e200) and a plane light
curve per plane (c2r_set_plane_curve: depths uniform, on a layer centre and one ulp either side, layer0 and depth0 above 0, a
dark gap, a depth horizon), in front of them fixed cases for the k_rates_curve instantiations no other test launches; the
setters are called in an order drawn per case.  tests/test_extension_fuzz_host.py proves on the CPU that every case of both
lists is well-posed.   python -m pytest tests -m gpu.   C2R_EXTFUZZ_CASES / C2R_EXTFUZZ_SEED / C2R_EXTFUZZ_CURVED_CASES
widen or move the lists; an id of the default list keeps its number.

One case is one test id.  The bar is np.array_equal with the printed spec as the tag: phih_grid, phihe_grid, phiheat, sum_nbox,
the rounds and the final box of every source, every open face's escape map and total, each plane's exit columns and exit
flux, the horizon loss per source == rim_reference.face_sum of the expected terms and their total, the rim terms of the
horizoned source swept last, and after the global pass the non-converged count, the four iteration-state arrays and the
temperature.  Two sums that the device adds in another order than their reference keep the bounds the project already has
for them (tests/test_gpu_plane_mix.py): c2r_get_plane_loss 1e-13 relative against math.fsum of the plane's terms, and
photon_loss(1) 1e-12 relative where mix_reference.has_loss_reference holds and no beam or horizon is set (with curves the
reference is the fsum of the curved per-source map totals and the planes' losses).
A second test over the ids of the curved list takes the curves off and puts them back on the same context, from the re-uploaded
state each time: what a batch's classification into k_rates / k_rates_beam / k_rates_curve, a source's learnt box, the tile
lists and a plane's record keep across the c2r_set_* calls.
Measured on one MI355X: the 28 ids of the default list take 4.6 s, references included; the first id, which also starts the
GPU runtime, 0.38 s, the slowest after it (several rounds on the 11 x 24 x 24 mesh) 0.33 s, the median 0.14 s -- beside 0.19 s
for the slowest id of tests/test_gpu_horizon_loss.py in the same run.  Most of an id is the oracle on the CPU.
With the curved list, measured on one MI355X: the file's 62 ids take 9.7 s.  The 28 ids of the default list 4.6 s as before
(first id 0.47 s, the slowest after it 0.35 s, the median 0.14 s); the 17 ids of the curved list 2.7 s (the slowest, several
rounds on the 24 x 24 x 24 mesh with z open, 0.29 s, the median 0.14 s); the 17 ids of
test_curves_come_off_and_go_back_on, three passes each on references the first test has composed, 2.1 s (the slowest 0.15 s,
the median 0.12 s).
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
SPECS = xf.full_list()
CURVED = [ic for ic, s in enumerate(SPECS) if "curves" in s]


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


def apply_settings(e, cfg, curved):
    """Horizons and beams, and for a case of the curved list the source curves and the plane curves too, in the case's drawn
    order: the setters keep each other's state."""
    for what in cfg["set_order"]:
        if what == "horizons":
            e.set_source_horizons(cfg["horizons"])
        elif what == "beams":
            e.set_source_beams(cfg["beams"])
        elif what == "curves" and curved:
            e.set_source_curves(cfg["curves"])
        elif what == "plane_curves" and curved:
            for p, plane in enumerate(cfg["planes"], start=1):
                e.set_plane_curve(p, plane["curve"])
    if curved:
        for ns, c in enumerate(cfg["curves"], start=1):
            assert e.source_curve(ns) == (([], [1.0]) if c is None else c), ns
        for p, plane in enumerate(cfg["planes"], start=1):
            assert e.plane_curve(p) == (([], [1.0], 0, 0.0) if plane["curve"] is None else plane["curve"]), p


def new_step(pkg, e, case):
    """The case's original state again, as a new time step would begin (run_route calls begin_step)."""
    ndens, xh, xhe, temp = case.region
    e.upload_state(pkg.Material(ndens, xh.copy(), xhe.copy(), None if temp is None else temp.copy(), not case.heat, 1.0e4, 1.0, case.reccoef))


def assert_rounds_grids_and_maps(e, got, mix, case, cfg, tag):
    """The rounds and the final box of every source, sum_nbox, the three grids and every escape map, bit for bit."""
    nsrc = len(case.flux)
    traces = [e.source_trace(ns) for ns in range(1, nsrc + 1)]
    print("rounds", [t["nbox"] for t in traces], "expected", [t[0] for t in mix["trace"]], "unbeamed", mix["oracle_nbox"])
    for ns, (tr, (nbox, lo, hi)) in enumerate(zip(traces, mix["trace"]), start=1):
        assert (tr["nbox"], tr["box_lo"], tr["box_hi"]) == (nbox, lo, hi), (ns, tr, tag)
    assert got["sum_nbox"] == mix["sum_nbox"], (got["sum_nbox"], mix["sum_nbox"], tag)
    for k in ("phih_grid", "phihe_grid") + (("phiheat",) if case.heat else ()):
        bad = int(np.count_nonzero(got[k] != mix[k]))
        print(k, "cells", got[k].size, "non-zero", int(np.count_nonzero(mix[k])), "differ", bad, "worst rel", float(np.max(rel_err(got[k], mix[k]))))
        assert np.array_equal(got[k], mix[k]), (k, bad, tag)
    if not case.heat:
        assert not got["phiheat"].any(), tag
    if cfg["maps"]:
        for f, want in mix["maps"].items():
            have = e.face_loss_map(f)
            assert have.shape == want.shape and np.array_equal(have, want), (f, tag)


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
    apply_settings(e, cfg, "curves" in spec)
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


@pytest.mark.parametrize("ic", CURVED)
def test_curves_come_off_and_go_back_on(pkg, orc, otables3, tables3, ic):
    """On one context: the case as drawn; then, from the re-uploaded state, every source and plane curve taken off -- the
    composition of the spec without curves, beams, horizons and planes kept; then the curves set again and the route 'plain' --
    the first composition.  Rounds, boxes, sum_nbox, the three grids and the escape maps bit for bit each time: nothing of a
    batch's classification, a source's learnt box, the tile lists or a plane's record outlives the call that changes it."""
    spec = SPECS[ic]
    tag = xf.tag(ic, spec)
    _progress("re-run " + tag)
    print(tag)
    case, cfg = xf.build(pkg, spec)
    mix = xf.compose_all(pkg, orc, otables3, case, spec)
    bare = xf.compose_all(pkg, orc, otables3, case, xf.uncurved(spec))
    nsrc, planes = len(case.flux), cfg["planes"]
    e = make_engine(pkg, tables3, case, planes, maps=cfg["maps"], batch=cfg["batch"])
    if cfg["horizon_loss"]:
        e.enable_horizon_loss()
    apply_settings(e, cfg, True)
    run_route(e, cfg, nsrc)
    assert_rounds_grids_and_maps(e, e.download_rates(), mix, case, cfg, ("as drawn", tag))
    new_step(pkg, e, case)
    e.set_source_curves(None)
    for p in range(1, len(planes) + 1):
        e.set_plane_curve(p, None)
    run_route(e, cfg, nsrc)
    assert_rounds_grids_and_maps(e, e.download_rates(), bare, case, cfg, ("curves off", tag))
    new_step(pkg, e, case)
    e.set_source_curves(cfg["curves"])
    for p, plane in enumerate(planes, start=1):
        e.set_plane_curve(p, plane["curve"])
    run_route(e, dict(cfg, route="plain"), nsrc)
    assert_rounds_grids_and_maps(e, e.download_rates(), mix, case, cfg, ("curves on again", tag))
    e.close()
    _progress(f"re-run of case {ic} done")
