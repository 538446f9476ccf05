"""tests/extension_fuzz_cases.py held to account on the CPU, before any GPU sees its cases.  Every check runs over the
default case list (C2R_EXTFUZZ_CASES / C2R_EXTFUZZ_SEED widen or move it), so a pass here says that the inputs of
tests/test_gpu_extension_fuzz.py are sound:

1. Well-posed: for every case with an open axis the oracle's results on the region -- all rate grids and the columns of the
   last source -- are the same bits from two periodic embeddings with different padding gas and a different open extent.
2. The fold: with beams, horizons and planes stripped, compose_all is the oracle's pass_all_sources on the embedding, cut to the
   region, bit for bit.  That licenses grid = grid + term_s in source order.
3. The predicates at the drawn edges: beam_reference.lit_offsets, horizon_reference.within_offsets and the rule of
   rim_reference.columns against the product's own headers compiled for the host (tests/horizon_harness.cpp,
   tests/rim_harness.cpp), for every beam, radius, dr and box of the list, every offset within 24 cells.  The lattice radii
   produce ties: some drawn radius has a cell with d2 == R2 exactly.
4. Coverage is a condition: the tallies are printed and asserted, and the committed seed was chosen so that they hold.
"""
import collections
import ctypes as C

import numpy as np
import pytest

import beam_reference as br
import extension_fuzz_cases as xf
import horizon_reference as hr
import mix_reference as mr
import rim_reference as rr
from test_gpu_plane_mix import otables3  # noqa: F401  (fixture: the oracle's tables with the two extra SEDs)
from test_horizon_loss_host import header_columns, rh  # noqa: F401  (fixture: csrc/c2ray_rim.hpp for the host)
from test_source_horizons_host import hh  # noqa: F401  (fixture: csrc/c2ray_horizon.hpp and c2ray_beam.hpp for the host)

SPECS = xf.case_list()
HALF = 24                                     # no offset of any box of the list is longer
INF = float("inf")


@pytest.fixture(scope="module")
def built(pkg):
    return [xf.build(pkg, spec) for spec in SPECS]


def test_the_list_is_seeded_and_plain():
    """The same seed gives the same list; a spec is made of plain Python values, so its repr is the whole case."""
    again = xf.case_list()
    assert [repr(s) for s in again] == [repr(s) for s in SPECS] and len(SPECS) == xf.NCASES + len(xf.FIXED)
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
        for ns, (beam, radius) in enumerate(zip(cfg["beams"], cfg["horizons"])):
            t = (ns, xf.tag(ic, spec))
            lit, within = br.lit_offsets(beam, case.dr, *o), hr.within_offsets(radius, case.dr, *o)
            assert np.array_equal(header_cut(hh, beam, None, case.dr), lit), t
            assert np.array_equal(header_cut(hh, None, radius, case.dr), within), t
            assert np.array_equal(header_cut(hh, beam, radius, case.dr), lit & within), t
            assert lit[HALF, HALF, HALF] and within[HALF, HALF, HALF], t
            checked += 1
            nbox, lo, hi = xf.expected_trace(case, ns, beam, radius)
            assert all(-HALF <= a <= 0 <= b <= HALF for a, b in zip(lo, hi)), t
            if radius is not None:
                assert hh.hh_horizon_R2(float(radius)) == float(hr.horizon_R2(radius)), t
            if spec["horizons"][ns]["radius_class"].startswith("lattice"):
                box = xf.box_offsets(*case.reach(ns))
                xs, ys, zs = (np.float64(case.dr[d]) * box[d].astype(np.float64) for d in range(3))
                ties += int(np.count_nonzero((xs * xs + ys * ys) + zs * zs == hr.horizon_R2(radius)) > 0)
            if xf.is_finite(radius):
                got, want = header_columns(rh, radius, case.dr, lo, hi, beam), rr.columns(radius, case.dr, lo, hi, beam)
                for k in ("col", "kstar", "face", "w"):
                    assert np.array_equal(got[k], want[k]), (k,) + t
                assert np.array_equal(got["cell"][want["kstar"] >= 0], want["cell"][want["kstar"] >= 0]), t
                rims += 1
    print("sources checked", checked, "rim boxes", rims, "lattice radii with a cell exactly on the sphere", ties)
    assert ties >= 1 and rims >= 5


# -- 4 ---------------------------------------------------------------------------------------------------------------------------
def tallies(built):
    """What the default list covers, from the specs and the built cases alone (no oracle)."""
    t = collections.OrderedDict()
    t["masks"] = collections.Counter(s["mask"] for s in SPECS)
    t["tiers"] = collections.Counter(s["tier"] for s in SPECS)
    t["routes"] = collections.Counter(s["route"] for s in SPECS)
    t["beam kinds"] = collections.Counter(b["kind"] for s in SPECS for b in s["beams"])
    t["cos_half"] = collections.Counter(b["cos_class"] for s in SPECS for b in s["beams"] if b["kind"])
    t["radius"] = collections.Counter(h["radius_class"] for s in SPECS for h in s["horizons"])
    t["heating"] = sum(s["heat"] for s in SPECS)
    t["three SEDs"] = sum(s["multi"] for s in SPECS)
    t["non-cubic"] = sum(not s["cubic"] for s in SPECS)
    t["gas"] = collections.Counter(s["gas"] for s in SPECS)
    t["with a plane"] = sum(bool(s["planes"]) for s in SPECS)
    t["plane kinds"] = collections.Counter(p["kind"] for s in SPECS for p in s["planes"])
    cut = lambda s: any(b["kind"] for b in s["beams"]) or any(h["radius_class"] not in ("none", "inf") for h in s["horizons"])
    t["plane and a beam or horizon"] = sum(bool(s["planes"]) and cut(s) for s in SPECS)
    t["an axis of 2 or 3 cells"] = sum(min(s["n"]) <= 3 for s in SPECS)
    t["two sources in one cell"] = sum(len({tuple(p) for p in s["srcpos"]}) < len(s["srcpos"]) for s in SPECS)
    t["one cell, different beams"] = 0
    beamed, partly, sheets = 0, 0, []
    for spec, (case, cfg) in zip(SPECS, built):
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
                                         for spec, (case, cfg) in zip(SPECS, built) for ns in range(len(case.flux)))
    t["photon_loss(1) has a reference"] = sum(mr.has_loss_reference(case) and all(b is None for b in cfg["beams"]) and
                                              not any(xf.is_finite(h) for h in cfg["horizons"]) for case, cfg in built)
    t["rejected draws"] = [r for s in SPECS for r in s["rejected"]]
    return t


def test_coverage_is_a_condition(pkg, orc, otables3, built):
    t = tallies(built)
    for k, v in t.items():
        print(f"{k}: {dict(v) if isinstance(v, collections.Counter) else v}")
    print("rejected draws in all:", len(t["rejected draws"]))
    if (xf.NCASES, xf.SEED) != (xf.DEFAULT_CASES, xf.DEFAULT_SEED):
        return                                              # a moved or widened list is anybody's: the conditions are the default's
    assert set(t["masks"]) == set(xf.MASKS)
    assert set(t["beam kinds"]) == {0, 1, 2} and set(t["cos_half"]) == set(xf.COS_CLASSES)
    assert set(t["radius"]) == set(xf.RADIUS_CLASSES)
    assert set(t["routes"]) == set(xf.ROUTES) and set(t["tiers"]) == {"A", "B"}
    assert 0 < t["heating"] < len(SPECS) and 0 < t["three SEDs"] < len(SPECS)
    assert t["with a plane"] >= 6 and t["plane and a beam or horizon"] >= 3 and set(t["plane kinds"]) == set(xf.PLANE_KINDS)
    assert t["an axis of 2 or 3 cells"] >= 4 and t["one cell, different beams"] >= 1
    assert 2 * t["of them partly lit"] >= t["beamed sources"] > 0
    assert sum(T % rr.BLOCK != 0 for T in t["rim sheets T"]) >= 2 and min(t["rim sheets T"]) < rr.BLOCK
    assert t["early end of the box loop"] >= 1 and t["photon_loss(1) has a reference"] >= 1
    losses = []
    for spec, (case, cfg) in zip(SPECS, built):
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
