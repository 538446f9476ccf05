"""tests/extension_fuzz_cases.py held to account on the CPU, before any GPU sees its cases.  Every check runs over the
default case list and the curved list behind it -- source and plane light curves -- (C2R_EXTFUZZ_CASES / C2R_EXTFUZZ_SEED /
C2R_EXTFUZZ_CURVED_CASES widen or move them), so a pass here says that the inputs of tests/test_gpu_extension_fuzz.py are sound:

1. Well-posed: for every case with an open axis the oracle's results on the region -- all rate grids and the columns of the
   last source -- are the same bits from two periodic embeddings with different padding gas and a different open extent.
2. The fold: with beams, horizons and planes stripped, compose_all is the oracle's pass_all_sources on the embedding, cut to the
   region, bit for bit.  That licenses grid = grid + term_s in source order.
3. The predicates at the drawn edges: beam_reference.lit_offsets, horizon_reference.within_offsets and the rule of
   rim_reference.columns against the product's own headers compiled for the host (tests/horizon_harness.cpp,
   tests/rim_harness.cpp), for every beam, radius, dr and box of the list, every offset within 24 cells.  The lattice radii
   produce ties: some drawn radius has a cell with d2 == R2 exactly.
4. Coverage is a condition: the tallies are printed and asserted, and the committed seed was chosen so that they hold.
5. The curved list leaves the default list where it was (a SHA-256 over its repr), and what the composer leans on for curves:
   plane_curve_reference.curve_pass without a curve is mix_reference.plane_alone and a curve of ones composes to the uncurved
   bits; a power of two scales a several-round oracle run exactly; on every intermediate box of a curved several-round source
   the smallest lit deciding loss term times the smallest factor is 10^3 above the threshold, which uses the unscaled flux;
   curve_reference.factor_offsets and plane_curve_reference.layer_factor against the product's headers compiled for the host,
   with a cell exactly on a drawn radius and a layer centre exactly on a drawn depth; and the coverage of the curved list.
Measured on one CPU host, same session and command (python -m pytest tests/test_extension_fuzz_host.py -q), three runs each:
the parent commit's file 8.1 / 10.8 / 10.9 s, this one 14.9 / 16.4 / 19.8 s with the default C2R_EXTFUZZ_CURVED_CASES = 10 -- 1.5
times by the medians, and the bound that chose the default is twice.  (With 12 the file takes 21 s: a draw with two eight-step
curves of factors that are no powers of two costs an oracle run per such factor and source.)
"""
import collections
import ctypes as C
import hashlib

import numpy as np
import pytest

import axis_boundary_cases as ab
import beam_reference as br
import curve_reference as cr
import extension_fuzz_cases as xf
import horizon_reference as hr
import mix_reference as mr
import plane_curve_reference as pcr
import rim_reference as rr
from test_gpu_plane_mix import otables3  # noqa: F401  (fixture: the oracle's tables with the two extra SEDs)
from test_gpu_source_horizons import THRESHOLD
from test_horizon_loss_host import header_columns, rh  # noqa: F401  (fixture: csrc/c2ray_rim.hpp for the host)
from test_plane_curve_host import harness_factors, pc  # noqa: F401  (fixture: csrc/c2ray_pcurve.hpp for the host)
from test_source_curves_host import _tables, ch  # noqa: F401  (fixture: csrc/c2ray_curve.hpp for the host)
from test_source_horizons_host import hh  # noqa: F401  (fixture: csrc/c2ray_horizon.hpp and c2ray_beam.hpp for the host)

SPECS = xf.full_list()
NOLD = len(xf.case_list())                    # the default list in front, the curved list from here on
OLD_DIGEST = "8137e89fa2257787040cdade947eadc8263a333d6731297d5ccd7e1e207683a0"      # SHA-256 of repr(case_list()), default list
HALF = 24                                     # no offset of any box of the list is longer
INF = float("inf")


@pytest.fixture(scope="module")
def built(pkg):
    return [xf.build(pkg, spec) for spec in SPECS]


def test_the_list_is_seeded_and_plain():
    """The same seed gives the same list; a spec is made of plain Python values, so its repr is the whole case."""
    again = xf.full_list()
    assert [repr(s) for s in again] == [repr(s) for s in SPECS]
    assert NOLD == xf.NCASES + len(xf.FIXED) and len(SPECS) == NOLD + xf.NCURVED + len(xf.FIXED_CURVED)
    assert not any(xf.has_curves(s) or "curves" in s or "set_order" in s for s in SPECS[:NOLD])
    if (xf.NCASES, xf.SEED) == (xf.DEFAULT_CASES, xf.DEFAULT_SEED):      # the curved list has not moved the default list
        assert hashlib.sha256(repr(SPECS[:NOLD]).encode()).hexdigest() == OLD_DIGEST
    if xf.NCURVED > 1:                                                   # draw_curved is draw and then the curves
        first = xf.draw(np.random.default_rng([xf.SEED, 1, 1]))
        mine = SPECS[NOLD + len(xf.FIXED_CURVED) + 1]
        assert all(repr(mine[k]) == repr(v) for k, v in first.items() if k not in ("planes", "rejected"))
        assert [{k: v for k, v in p.items() if k != "curve"} for p in mine["planes"]] == first["planes"]
    assert repr(xf.draw(np.random.default_rng(xf.SEED + 1))) == repr(SPECS[len(xf.FIXED) + 1]) if xf.NCASES > 1 else True

    def plain(x):
        if isinstance(x, (list, tuple)):
            return all(plain(y) for y in x)
        if isinstance(x, dict):
            return all(isinstance(k, str) and plain(v) for k, v in x.items())
        return x is None or type(x) in (bool, int, float, str)

    for ic, spec in enumerate(SPECS):
        assert plain(spec), xf.tag(ic, spec)
        assert max(spec["n"]) <= 24 and 1 <= len(spec["flux"]) <= 4 and 1 <= spec["batch"] <= 8, xf.tag(ic, spec)


# -- 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ic", range(len(SPECS)))
def test_well_posed_on_two_embeddings(pkg, orc, otables3, built, ic):
    spec, (case, _) = SPECS[ic], built[ic]
    case.check_embedding(case.m)
    other = xf.other_embedding(pkg, case, spec)
    if other is None:
        assert all(case.periodic) and case.m == case.n      # the embedding is the mesh itself: nothing to compare
        return
    m2, big2 = other
    assert m2 != case.m
    a = case.oracle_pass(pkg, orc, otables3)
    b = case.oracle_pass(pkg, orc, otables3, m=m2, big=big2)
    for k in xf.GRIDS + ("coldensh_out", "coldenshe_out"):
        assert np.array_equal(a[k], b[k]), (k, xf.tag(ic, spec))
    assert a["phih_grid"].any()


# -- 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ic", range(len(SPECS)))
def test_fold_without_features_is_the_oracles_pass(pkg, orc, otables3, built, ic):
    spec, (case, _) = SPECS[ic], built[ic]
    bare = xf.compose_all(pkg, orc, otables3, case, xf.stripped(spec))
    want = case.oracle_pass(pkg, orc, otables3)
    assert all(bare["same_cells"]), (bare["oracle_nbox"], xf.tag(ic, spec))
    for k in xf.GRIDS:
        assert np.array_equal(bare[k], want[k]), (k, xf.tag(ic, spec))
    assert bare["sum_nbox"] == case.expected_rounds() if spec["tier"] == "B" else bare["sum_nbox"] == len(case.flux)
    if all(case.periodic):
        assert bare["sum_nbox"] == want["sum_nbox"], xf.tag(ic, spec)
    for ns in range(len(case.flux)):                        # unbeamed, the final box is the reach
        assert (bare["trace"][ns][1], bare["trace"][ns][2]) == tuple(case.reach(ns)), xf.tag(ic, spec)


# -- 3 ---------------------------------------------------------------------------------------------------------------------------
def cube_offsets():
    r = np.arange(-HALF, HALF + 1)
    dk, dj, di = np.meshgrid(r, r, r, indexing="ij")
    return di, dj, dk


def header_cut(hh, beam, radius, dr):
    kind, axis, cos_half = (0, (0.0, 0.0, 0.0), 0.0) if beam is None else beam
    w = 2 * HALF + 1
    out = (C.c_ubyte * (w * w * w))()
    hh.hh_cut_cube(int(kind), (C.c_double * 3)(*axis), float(cos_half), INF if radius is None else float(radius),
                   (C.c_double * 3)(*dr), HALF, out)
    return np.frombuffer(out, dtype=np.uint8).reshape(w, w, w).astype(bool)


def test_predicates_against_the_headers(hh, rh, built):
    o = cube_offsets()
    ties, checked, rims = 0, 0, 0
    for ic, (spec, (case, cfg)) in enumerate(zip(SPECS, built)):
        for ns, (beam, radius, curve) in enumerate(zip(cfg["beams"], cfg["horizons"], cfg["curves"])):
            t = (ns, xf.tag(ic, spec))
            lit, within = br.lit_offsets(beam, case.dr, *o), hr.within_offsets(radius, case.dr, *o)
            assert np.array_equal(header_cut(hh, beam, None, case.dr), lit), t
            assert np.array_equal(header_cut(hh, None, radius, case.dr), within), t
            assert np.array_equal(header_cut(hh, beam, radius, case.dr), lit & within), t
            assert lit[HALF, HALF, HALF] and within[HALF, HALF, HALF], t
            checked += 1
            nbox, lo, hi = xf.expected_trace(case, ns, beam, radius, curve)
            assert all(-HALF <= a <= 0 <= b <= HALF for a, b in zip(lo, hi)), t
            if radius is not None:
                assert hh.hh_horizon_R2(float(radius)) == float(hr.horizon_R2(radius)), t
            if spec["horizons"][ns]["radius_class"].startswith("lattice"):
                box = xf.box_offsets(*case.reach(ns))
                xs, ys, zs = (np.float64(case.dr[d]) * box[d].astype(np.float64) for d in range(3))
                ties += int(ic < NOLD and np.count_nonzero((xs * xs + ys * ys) + zs * zs == hr.horizon_R2(radius)) > 0)
            if xf.is_finite(radius):
                got, want = header_columns(rh, radius, case.dr, lo, hi, beam), rr.columns(radius, case.dr, lo, hi, beam)
                for k in ("col", "kstar", "face", "w"):
                    assert np.array_equal(got[k], want[k]), (k,) + t
                assert np.array_equal(got["cell"][want["kstar"] >= 0], want["cell"][want["kstar"] >= 0]), t
                rims += int(ic < NOLD)
    print("sources checked", checked, "in the default list: rim boxes", rims, "lattice radii with a cell exactly on the sphere", ties)
    assert ties >= 1 and rims >= 5


# -- 4 ---------------------------------------------------------------------------------------------------------------------------
def tallies(specs, built):
    """What the default list covers, from the specs and the built cases alone (no oracle)."""
    t = collections.OrderedDict()
    t["masks"] = collections.Counter(s["mask"] for s in specs)
    t["tiers"] = collections.Counter(s["tier"] for s in specs)
    t["routes"] = collections.Counter(s["route"] for s in specs)
    t["beam kinds"] = collections.Counter(b["kind"] for s in specs for b in s["beams"])
    t["cos_half"] = collections.Counter(b["cos_class"] for s in specs for b in s["beams"] if b["kind"])
    t["radius"] = collections.Counter(h["radius_class"] for s in specs for h in s["horizons"])
    t["heating"] = sum(s["heat"] for s in specs)
    t["three SEDs"] = sum(s["multi"] for s in specs)
    t["non-cubic"] = sum(not s["cubic"] for s in specs)
    t["gas"] = collections.Counter(s["gas"] for s in specs)
    t["with a plane"] = sum(bool(s["planes"]) for s in specs)
    t["plane kinds"] = collections.Counter(p["kind"] for s in specs for p in s["planes"])
    cut = lambda s: any(b["kind"] for b in s["beams"]) or any(h["radius_class"] not in ("none", "inf") for h in s["horizons"])
    t["plane and a beam or horizon"] = sum(bool(s["planes"]) and cut(s) for s in specs)
    t["an axis of 2 or 3 cells"] = sum(min(s["n"]) <= 3 for s in specs)
    t["two sources in one cell"] = sum(len({tuple(p) for p in s["srcpos"]}) < len(s["srcpos"]) for s in specs)
    t["one cell, different beams"] = 0
    beamed, partly, sheets = 0, 0, []
    for spec, (case, cfg) in zip(specs, built):
        for ns, beam in enumerate(cfg["beams"]):
            if beam is not None:
                f = float(br.lit_cells(case, ns, beam).mean())
                beamed, partly = beamed + 1, partly + (0.0 < f < 1.0)
            for other in range(ns):
                if tuple(spec["srcpos"][ns]) == tuple(spec["srcpos"][other]) and cfg["beams"][ns] != cfg["beams"][other]:
                    t["one cell, different beams"] += 1
            if cfg["horizon_loss"] and xf.is_finite(cfg["horizons"][ns]):
                _, lo, hi = xf.expected_trace(case, ns, beam, cfg["horizons"][ns])
                sheets.append(rr.total(lo, hi))
    t["beamed sources"], t["of them partly lit"] = beamed, partly
    t["rim sheets T"] = sorted(sheets)
    t["early end of the box loop"] = sum(xf.expected_trace(case, ns, cfg["beams"][ns], cfg["horizons"][ns])[0] <
                                         xf.expected_trace(case, ns, None, None)[0]
                                         for spec, (case, cfg) in zip(specs, built) for ns in range(len(case.flux)))
    t["photon_loss(1) has a reference"] = sum(mr.has_loss_reference(case) and all(b is None for b in cfg["beams"]) and
                                              not any(xf.is_finite(h) for h in cfg["horizons"]) for case, cfg in built)
    t["rejected draws"] = [r for s in specs for r in s["rejected"]]
    return t


def test_coverage_is_a_condition(pkg, orc, otables3, built):
    t = tallies(SPECS[:NOLD], built[:NOLD])
    print("the default list")
    for k, v in t.items():
        print(f"{k}: {dict(v) if isinstance(v, collections.Counter) else v}")
    print("rejected draws in all:", len(t["rejected draws"]))
    if (xf.NCASES, xf.SEED) != (xf.DEFAULT_CASES, xf.DEFAULT_SEED):
        return                                              # a moved or widened list is anybody's: the conditions are the default's
    assert set(t["masks"]) == set(xf.MASKS)
    assert set(t["beam kinds"]) == {0, 1, 2} and set(t["cos_half"]) == set(xf.COS_CLASSES)
    assert set(t["radius"]) == set(xf.RADIUS_CLASSES)
    assert set(t["routes"]) == set(xf.ROUTES) and set(t["tiers"]) == {"A", "B"}
    assert 0 < t["heating"] < NOLD and 0 < t["three SEDs"] < NOLD
    assert t["with a plane"] >= 6 and t["plane and a beam or horizon"] >= 3 and set(t["plane kinds"]) == set(xf.PLANE_KINDS)
    assert t["an axis of 2 or 3 cells"] >= 4 and t["one cell, different beams"] >= 1
    assert 2 * t["of them partly lit"] >= t["beamed sources"] > 0
    assert sum(T % rr.BLOCK != 0 for T in t["rim sheets T"]) >= 2 and min(t["rim sheets T"]) < rr.BLOCK
    assert t["early end of the box loop"] >= 1 and t["photon_loss(1) has a reference"] >= 1
    losses = []
    for spec, (case, cfg) in zip(SPECS[:NOLD], built[:NOLD]):
        if cfg["horizon_loss"]:
            mix = xf.compose_all(pkg, orc, otables3, case, spec)
            losses += [float(x) for x in mix["horizon_loss"] if x > 0]
    print("sources with an expected horizon loss above 0:", len(losses), sorted(losses))
    assert len(losses) >= 5


def test_every_case_composes(pkg, orc, otables3, built):
    """compose_all runs for every case of the list, the oracle traced what the product is expected to trace, and the features
    change what a case without them gives wherever some cell is cut."""
    for ic, (spec, (case, cfg)) in enumerate(zip(SPECS, built)):
        mix = xf.compose_all(pkg, orc, otables3, case, spec)
        assert all(mix["same_cells"]), (mix["oracle_nbox"], xf.tag(ic, spec))
        assert mix["sum_nbox"] >= len(case.flux) and all(np.isfinite(mix[k]).all() for k in xf.GRIDS), xf.tag(ic, spec)
        for ns, (nbox, lo, hi) in enumerate(mix["trace"]):
            assert (lo, hi) == tuple(rr.final_box(case, ns, nbox)), xf.tag(ic, spec)
        assert sorted(mix["maps"]) == [f for f in range(6) if not case.periodic[f // 2]], xf.tag(ic, spec)


# -- 5 ---------------------------------------------------------------------------------------------------------------------------
CURVED = range(NOLD, len(SPECS))
PLANE_KEYS = xf.GRIDS + ("exit", "terms", "exit_flux")


def all_ones(curve):
    return curve is not None and all(f == 1.0 for f in curve[1])


def test_licence_for_the_swap(pkg, orc, otables3, built):
    """compose_all takes a curved plane from plane_curve_reference.curve_pass and an uncurved one from mix_reference.plane_alone:
    without a curve the two agree bit for bit, for every plane of both lists.  A source whose factors are all 1.0 composes to
    what it composes to without its curve."""
    planes = ones = 0
    for ic, (spec, (case, cfg)) in enumerate(zip(SPECS, built)):
        for p, plane in enumerate(cfg["planes"], start=1):
            a, b = xf.curve_pass(orc, otables3, case, plane, None), mr.plane_alone(orc, otables3, case, plane)
            for k in PLANE_KEYS:
                if k in b:
                    assert np.array_equal(a[k], b[k]), (k, p, xf.tag(ic, spec))
            assert a["loss"] == b["loss"], (p, xf.tag(ic, spec))
            planes += 1
        if any(all_ones(c) for c in cfg["curves"]):
            bare = dict(spec, curves=[None if all_ones(c) else s for c, s in zip(cfg["curves"], spec["curves"])])
            a, b = xf.compose_all(pkg, orc, otables3, case, spec), xf.compose_all(pkg, orc, otables3, case, bare)
            for k in xf.GRIDS:
                assert np.array_equal(a[k], b[k]), (k, xf.tag(ic, spec))
            assert a["trace"] == b["trace"] and all(np.array_equal(a["maps"][f], b["maps"][f]) for f in a["maps"]), xf.tag(ic, spec)
            assert np.array_equal(a["horizon_loss"], b["horizon_loss"]), xf.tag(ic, spec)
            ones += 1
    print("planes without a curve through both references", planes, "cases with a curve of ones", ones)
    assert planes >= 6 and (ones >= 1 or xf.NCURVED != xf.DEFAULT_CURVED)


def test_a_power_of_two_scales_a_tier_b_run_exactly(pkg, orc, otables3, built):
    """The premise of tier B's curves: a real oracle run with the flux times a power of two is the factor-1 term times it."""
    for ic in CURVED:
        spec, (case, cfg) = SPECS[ic], built[ic]
        if spec["tier"] != "B":
            continue
        for ns, curve in enumerate(cfg["curves"], start=1):
            fs = [] if curve is None else [f for f in curve[1] if f not in (0.0, 1.0)]
            if fs:
                key = xf.case_key(spec)
                base, nb, loss, _ = br.source_alone(pkg, orc, otables3, case, key, ns)
                grids, nb_f, loss_f, _ = cr.source_scaled(pkg, orc, otables3, case, key, ns, fs[0])
                print(xf.tag(ic, spec), "source", ns, "factor", fs[0], "rounds", nb, nb_f)
                assert xf.is_pow2(fs[0]) and nb_f == nb and loss_f == fs[0] * loss
                for k in xf.GRIDS:
                    assert np.array_equal(grids[k], fs[0] * base[k]) and (k == "phiheat" or base[k].any()), (k, xf.tag(ic, spec))
                return
    assert xf.NCURVED != xf.DEFAULT_CURVED, "no tier B source with a factor other than 0 and 1"


def test_tier_b_rounds_with_a_curve(pkg, orc, otables3, built):
    """The product's threshold uses the unscaled flux (csrc/c2ray_curve.hpp), so 'the loop goes on exactly while some lit cell
    lies on a face that decides' needs every such cell's scaled term far above it: on every intermediate box of every curved
    tier B source the smallest lit deciding term times the smallest non-zero factor exceeds THRESHOLD x flux by 10^3."""
    boxes, worst = 0, float("inf")
    for ic in CURVED:
        spec, (case, cfg) = SPECS[ic], built[ic]
        if spec["tier"] != "B":
            continue
        key = xf.case_key(spec)
        for ns, curve in enumerate(cfg["curves"]):
            if curve is None:
                continue
            br.source_alone(pkg, orc, otables3, case, key, ns + 1)
            xf.compose_all(pkg, orc, otables3, case, spec)                 # (hands rim_reference the oracle's run)
            flux = float(case.flux[ns]) * case.s_star
            if case.pl is not None:
                flux = flux + float(case.pl[ns]) * case.pl_s_star + float(case.qpl[ns]) * case.qpl_s_star
            fmin = min(f for f in curve[1] if f != 0.0) if any(curve[1]) else 0.0
            last = xf.expected_trace(case, ns, cfg["beams"][ns], cfg["horizons"][ns], curve)[0]
            for nbox in range(1, last):
                o, decides = xf.deciding_cells(case, ns, nbox)
                lit = decides & hr.lit_offsets(cfg["beams"][ns], cfg["horizons"][ns], case.dr, *o) & (cr.factor_offsets(curve, case.dr, *o) != 0.0)
                assert lit.any(), (ns, nbox, xf.tag(ic, spec))
                terms = []
                for cell in zip(o[0][lit], o[1][lit], o[2][lit]):
                    po, vol_ph = rr.cell_photo_out_vol(pkg, orc, otables3, case, key, ns, tuple(int(x) for x in cell))
                    terms.append(po * float(case.vol) / vol_ph)
                ratio = min(terms) * fmin / (THRESHOLD * flux)
                print("case", ic, "source", ns + 1, "box", nbox, "lit deciding cells", len(terms), "smallest term x smallest factor / (threshold x flux)", ratio)
                assert ratio >= 1.0e3, (ns, nbox, ratio, xf.tag(ic, spec))
                boxes, worst = boxes + 1, min(worst, ratio)
    print("intermediate boxes of curved tier B sources", boxes, "worst ratio", worst)
    assert boxes >= 1 or xf.NCURVED != xf.DEFAULT_CURVED


def test_curve_predicates_against_the_headers(ch, pc, built):
    """curve_reference.factor_offsets against csrc/c2ray_curve.hpp for every drawn source curve, every offset within 24 cells;
    plane_curve_reference.layer_factor against csrc/c2ray_pcurve.hpp for every drawn plane curve and layer.  Some drawn radius
    has a cell with d2 == R2 exactly, some drawn depth equals a layer centre exactly."""
    o = cube_offsets()
    w = 2 * HALF + 1
    curves = planes = ties = centres = 0
    for ic in CURVED:
        spec, (case, cfg) = SPECS[ic], built[ic]
        for ns, curve in enumerate(cfg["curves"]):
            if curve is None:
                continue
            out = (C.c_double * (w * w * w))()
            n, r, f = _tables(curve)
            ch.ch_factor_cube(n, r, f, (C.c_double * 3)(*case.dr), HALF, out)
            got = np.frombuffer(out, dtype=np.float64).reshape(w, w, w)
            assert np.array_equal(got, cr.factor_offsets(curve, case.dr, *o)), (ns, xf.tag(ic, spec))
            assert all(ch.ch_curve_R2(float(x)) == float(cr.curve_R2(x)) for x in curve[0]), (ns, xf.tag(ic, spec))
            box = xf.box_offsets(*case.reach(ns))
            xs, ys, zs = (np.float64(case.dr[d]) * box[d].astype(np.float64) for d in range(3))
            d2 = (xs * xs + ys * ys) + zs * zs
            ties += int(any(np.count_nonzero(d2 == cr.curve_R2(x)) > 0 for x in curve[0] if x > 0.0))
            curves += 1
        for p, plane in zip(spec["planes"], cfg["planes"]):
            if plane["curve"] is None:
                continue
            na, path = case.n[plane["axis"]], pcr.plane_path(case.dr, plane["axis"], plane.get("tilt"))
            want = np.array([pcr.layer_factor(plane["curve"], m, path) for m in range(na)])
            assert np.array_equal(harness_factors(pc, plane["curve"], path, na), want), (plane["curve"], xf.tag(ic, spec))
            depths, _, layer0, depth0 = pcr.unpack(plane["curve"])
            centres += int(any(pcr.layer_depth(depth0, layer0, m, path) in depths for m in range(na)))
            planes += 1
    print("source curves checked", curves, "with a cell exactly on a radius", ties, "plane curves checked", planes, "with a centre exactly on a depth", centres)
    assert (ties >= 1 and centres >= 1) or xf.NCURVED != xf.DEFAULT_CURVED


def curved_tallies(built):
    """What the curved list covers, from the specs and the built cases alone (no oracle)."""
    specs, cases = [SPECS[ic] for ic in CURVED], [built[ic] for ic in CURVED]
    t = collections.OrderedDict()
    bent = lambda s: any(c is not None and any(f != 1.0 for f in c["factors"]) for c in s["curves"])
    t["(heating, three SEDs, an open axis) with a curve that is not all ones"] = collections.Counter(
        (s["heat"], s["multi"], bool(s["mask"])) for s in specs if bent(s))
    t["source curve classes"] = collections.Counter("none" if c is None else c["cls"] for s in specs for c in s["curves"])
    t["curve radius classes"] = collections.Counter(h["radius_class"] for s in specs for c in s["curves"] if c for h in c["radii"])
    t["curve steps"] = collections.Counter(len(c["radii"]) for s in specs for c in s["curves"] if c)
    t["plane curve classes"] = collections.Counter("none" if p["curve"] is None else p["curve"]["cls"] for s in specs for p in s["planes"])
    t["curved plane kinds"] = collections.Counter(p["kind"] + (", tilted" if p["kind"] == "mapped" and "tilt" in p else "")
                                                  for s in specs for p in s["planes"] if p["curve"])
    t["plane curves with layer0 > 0 and depth0 > 0"] = sum(p["curve"]["layer0"] > 0 and p["curve"]["depth0"] > 0
                                                           for s in specs for p in s["planes"] if p["curve"])
    t["centre nudges"] = collections.Counter(d["nudge"] for s in specs for p in s["planes"] if p["curve"] for d in p["curve"]["depths"]
                                             if d["kind"] == "centre")
    t["routes"] = collections.Counter(s["route"] for s in specs)
    t["tiers"] = collections.Counter(s["tier"] for s in specs)
    t["first setter"] = collections.Counter(s["set_order"][0] for s in specs)
    t["a curved and an uncurved source in one batch"] = sum(
        any(len({c is None for c in s["curves"][a:a + s["batch"]]}) == 2 for a in range(0, len(s["curves"]), s["batch"])) for s in specs)
    t["two sources in one cell, one curved"] = sum(any(tuple(s["srcpos"][a]) == tuple(s["srcpos"][b]) and (s["curves"][a] or s["curves"][b])
                                                       for a in range(len(s["flux"])) for b in range(a)) for s in specs)
    t["a curved plane with a curved point source"] = sum(any(p["curve"] for p in s["planes"]) and any(s["curves"]) for s in specs)
    t["an axis of 2 or 3 cells with a curved source"] = sum(min(s["n"]) <= 3 and any(s["curves"]) for s in specs)
    t["curved tier B cases"] = sum(s["tier"] == "B" and any(s["curves"]) for s in specs)
    t["beam, horizon, curve, the loss on, a rim face removed"] = 0
    t["open-face cells dark by the curve alone"] = 0
    t["tier B: early end of the box loop by the curve alone"] = 0
    for spec, (case, cfg) in zip(specs, cases):
        early = False
        for ns, (beam, radius, curve) in enumerate(zip(cfg["beams"], cfg["horizons"], cfg["curves"])):
            if curve is None:
                continue
            nbox, lo, hi = xf.expected_trace(case, ns, beam, radius, curve)
            early = early or nbox < xf.expected_trace(case, ns, beam, radius)[0]
            fac = cr.factors_of(curve)
            if beam is not None and xf.is_finite(radius) and cfg["horizon_loss"]:
                rule = rr.columns(radius, case.dr, lo, hi, beam)
                shell = cr.shell_offsets(curve, case.dr, rule["cell"][:, 0], rule["cell"][:, 1], rule["cell"][:, 2])
                t["beam, horizon, curve, the loss on, a rim face removed"] += int((rule["face"] & (fac[shell] == 0.0)).any())
            di, dj, dk = br.offsets(case.n, case.srcpos[ns], case.periodic)
            face = np.zeros(di.shape, dtype=bool)
            for d, m1 in enumerate(np.meshgrid(*(np.arange(1, case.n[a] + 1) for a in (2, 1, 0)), indexing="ij")[::-1]):
                if not case.periodic[d]:
                    face |= (m1 == 1) | (m1 == case.n[d])
            lit = br.lit_cells(case, ns, beam) & hr.within_cells(case, ns, radius) & xf.inside_cells(case, ns, lo, hi)
            t["open-face cells dark by the curve alone"] += int((face.reshape(-1) & lit & (cr.factor_cells(case, ns, curve) == 0.0)).sum())
        t["tier B: early end of the box loop by the curve alone"] += int(spec["tier"] == "B" and early)
    return t


def test_curved_coverage_is_a_condition(built):
    print("the curved list, by the default list's tallies")
    for k, v in tallies([SPECS[ic] for ic in CURVED], [built[ic] for ic in CURVED]).items():
        print(f"{k}: {dict(v) if isinstance(v, collections.Counter) else v}")
    t = curved_tallies(built)
    print("the curved list")
    for k, v in t.items():
        print(f"{k}: {dict(v) if isinstance(v, collections.Counter) else v}")
    combos = t["(heating, three SEDs, an open axis) with a curve that is not all ones"]
    for heat, multi, some_open in ((False, True, False), (False, True, True), (True, False, True), (True, True, True)):
        print("k_rates_curve<%s, %s, %s>: cases" % ("heating" if heat else "isothermal", "three SEDs" if multi else "one SED",
                                                     "open" if some_open else "periodic"), combos[(heat, multi, some_open)])
    if (xf.NCURVED, xf.SEED) != (xf.DEFAULT_CURVED, xf.DEFAULT_SEED):
        return                                              # a moved or widened list is anybody's: the conditions are the default's
    assert len(combos) == 8 and all(combos.values())
    assert set(t["source curve classes"]) == set(xf.CURVE_CLASSES) and set(t["curve radius classes"]) == set(xf.CURVE_RADIUS_CLASSES)
    assert 8 in t["curve steps"] and 0 in t["curve steps"]
    assert set(t["plane curve classes"]) == set(xf.PLANE_CURVE_CLASSES) and t["plane curves with layer0 > 0 and depth0 > 0"] >= 1
    assert set(t["centre nudges"]) == {-1, 0, 1}
    assert set(t["curved plane kinds"]) == {"normal", "tilted", "mapped", "mapped, tilted"}
    assert set(t["routes"]) == set(xf.ROUTES) and set(t["first setter"]) == set(xf.SETTERS)
    assert t["a curved and an uncurved source in one batch"] >= 2
    assert t["beam, horizon, curve, the loss on, a rim face removed"] >= 2
    assert t["open-face cells dark by the curve alone"] >= 1
    assert t["curved tier B cases"] >= 2 and t["tier B: early end of the box loop by the curve alone"] >= 1
    assert t["a curved plane with a curved point source"] >= 3
    assert t["an axis of 2 or 3 cells with a curved source"] >= 1 and t["two sources in one cell, one curved"] >= 1
