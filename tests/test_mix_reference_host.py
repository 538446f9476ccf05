"""tests/mix_reference.py held to account on the CPU, before any GPU sees it: the composition of several planes and point
sources in one pass returns what its parts return where only one part is there, changes no bit for a plane without flux,
depends on the order the header documents, and its plane part is what the product's own per-plane host harnesses
(tests/plane_harness.cpp, tests/oblique_harness.cpp, tests/flux_harness.cpp) give when they add into one array in plane order.
The generator of tests/test_gpu_plane_mix.py's random cases is checked here too: the default seed redraws at most a quarter.

Measured on the CPU: the whole file, 18 tests, takes 7 s (about 10 s more where the three harnesses have to be compiled first).
"""
import ctypes as C
import math

import numpy as np
import pytest

import face_loss_reference as fl
import mix_reference as mx
import plane_reference as pr
from test_flux_reference_host import fx  # noqa: F401  (fixtures: the three host harnesses with their tables set)
from test_gpu_plane_mix import otables3  # noqa: F401  (fixture: the oracle's tables with the two extra SEDs)
from test_oblique_reference_host import ob as obl  # noqa: F401
from test_plane_reference_host import ph  # noqa: F401

dp = C.POINTER(C.c_double)
GRIDS = ("phih_grid", "phihe_grid", "phiheat")


def _p(a):
    return a.ctypes.data_as(dp)


@pytest.fixture(scope="module")
def case_a(pkg):
    return mx.case_a(pkg)


@pytest.fixture(scope="module")
def mix_a(pkg, orc, otables, case_a):
    return mx.compose(pkg, orc, otables, case_a, mx.PLANES_A, "mix_a")


def same_grids(a, b):
    return all(np.array_equal(a[k], b[k]) for k in GRIDS)


def test_the_cells_are_no_cubes_and_the_embedding_holds(pkg, case_a):
    d = case_a.dr[0]
    assert case_a.dr == (d, 1.25 * d, 0.75 * d) and case_a.vol == d * (1.25 * d) * (0.75 * d)
    assert case_a.n == (11, 11, 11) and case_a.m == (11, 11, 24) and case_a.periodic == (True, True, False)
    for mask, (n, m) in mx.MESHES.items():
        c = mx.make_case(pkg, mask, [(1, 1, 1)], [1.0e7])
        assert c.n == n and c.m == m and c.periodic == tuple(ax not in mask for ax in "xyz")


@pytest.mark.parametrize("kind", ["plain", "tilted", "mapped", "tilted_mapped"])
def test_one_plane_and_no_point_source_is_the_single_plane_module(pkg, orc, otables, kind):
    """One plane, NumSrc = 0: grids, exit columns, exit flux, terms, loss and the far face's map are the matching module's."""
    case = mx.make_case(pkg, "xy", np.zeros((0, 3)), np.zeros(0))
    plane = dict(axis=0, from_high=1, normflux=mx.FLUX)
    if "tilted" in kind:
        plane["tilt"] = mx.TILT
    if "mapped" in kind:
        plane["fmap"] = mx.make_map(case, 0, 5)
    alone = mx.plane_alone(orc, otables, case, plane)
    mix = mx.compose(pkg, orc, otables, case, [plane], "one_" + kind)
    assert same_grids(mix, alone) and mix["sum_nbox"] == 0 and mix["planes"] == [1] and mix["sources"] == []
    assert mix["plane"][1]["loss"] == alone["loss"] and np.array_equal(mix["plane"][1]["exit"], alone["exit"])
    if "mapped" in kind:
        assert np.array_equal(mix["plane"][1]["exit_flux"], alone["exit_flux"])
    assert np.array_equal(mix["maps"][0], alone["terms"].reshape(24, 11)) and alone["terms"].any()
    assert not any(mix["maps"][f].any() for f in (1, 2, 3)) and sorted(mix["maps"]) == [0, 1, 2, 3]
    assert np.all(alone["phih_grid"] >= 0) and alone["phih_grid"].any()


@pytest.mark.parametrize("mask", ["z", "xyz"])
def test_no_plane_is_the_oracles_pass(pkg, orc, otables, mask):
    """A zero-seeded state and no plane: the do_source loop equals orc.pass_all_sources on all grids, on sum_nbox and on the
    loss, bit for bit (the oracle's own photon_loss(1) on the embedding, 0 + loss_1 + loss_2 + ...).  Beside that, the sources'
    kept terms are face_loss_reference's; with all axes open their sum is the reference of the PRODUCT's photon_loss(1)."""
    case = mx.make_case(pkg, mask, [(1, 1, 1), (11, 11, 11), (5, 11, 1), (6, 6, 6)], mx.FLUX_E)
    mix = mx.compose(pkg, orc, otables, case, [], "none_" + mask)
    want = case.oracle_pass(pkg, orc, otables)
    assert same_grids(mix, want) and mix["oracle_sum_nbox"] == want["sum_nbox"] == 4 and mix["nbox"] == [1, 1, 1, 1]
    assert mix["oracle_loss"] == want["photon_loss"] and want["photon_loss"] > 0
    assert mix["sum_nbox"] == 4 and all(mix["same_cells"])
    maps, _ = fl.expected(pkg, orc, otables, case, "none_" + mask)
    assert sorted(maps) == sorted(mix["maps"]) and all(np.array_equal(maps[f], mix["maps"][f]) for f in maps)
    if mask == "xyz":
        assert mix["loss"] is not None and abs(mix["loss"] - fl.total_of(maps)) <= 1e-15 * mix["loss"]
    else:                       # the faces of the periodic axes at +-N/2 lose photons that no map holds
        assert mix["loss"] is None
    assert want["phih_grid"].any()


def test_a_plane_without_flux_changes_no_bit(pkg, orc, otables, case_a, mix_a):
    """A third plane whose three fluxes are 0.0, in front of the others: every rate is +0.0 and no grid, map or loss changes."""
    dark = dict(axis=2, from_high=0, normflux=[0.0, 0.0, 0.0])
    mix = mx.compose(pkg, orc, otables, case_a, [dark] + mx.PLANES_A, "mix_a")
    assert same_grids(mix, mix_a) and mix["sum_nbox"] == mix_a["sum_nbox"]
    assert all(np.array_equal(mix["maps"][f], mix_a["maps"][f]) for f in mix_a["maps"])
    assert mix["plane"][1]["loss"] == 0.0 and not mix["plane"][1]["terms"].any() and not mix["plane"][1]["phih_grid"].any()
    assert mix["plane"][2]["loss"] == mix_a["plane"][1]["loss"] and mix["plane"][3]["loss"] == mix_a["plane"][2]["loss"]


def test_the_order_of_the_planes_matters(pkg, orc, otables, case_a, mix_a):
    """Two planes alone cannot tell their order: (0 + a) + b and (0 + b) + a are the same IEEE sum, so case a's list composed
    as (2, 1) has the bits of (1, 2) -- asserted, so that nobody looks for teeth there.  With a third plane on the same mesh
    the order shows: (1, 3, 2) differs from (1, 2, 3) in some cell of every rate grid."""
    swapped = mx.compose(pkg, orc, otables, case_a, mx.PLANES_A, "mix_a", plane_order=(2, 1))
    assert same_grids(swapped, mix_a)
    three = mx.compose(pkg, orc, otables, case_a, mx.PLANES_A3, "mix_a")
    other = mx.compose(pkg, orc, otables, case_a, mx.PLANES_A3, "mix_a", plane_order=(1, 3, 2))
    differ = {k: int(np.count_nonzero(three[k] != other[k])) for k in ("phih_grid", "phihe_grid")}
    print("cells whose bits depend on the planes' order:", differ)
    assert differ["phih_grid"] > 0 and differ["phihe_grid"] > 0
    assert np.allclose(three["phih_grid"], other["phih_grid"], rtol=1e-14, atol=0.0)


def test_planes_before_point_sources_matters(pkg, orc, otables, case_a, mix_a):
    """Case a's two planes folded after the four point sources instead of before: other bits in some cell, the same values to
    rounding."""
    after = mx.compose(pkg, orc, otables, case_a, mx.PLANES_A, "mix_a", planes_last=True)
    differ = {k: int(np.count_nonzero(after[k] != mix_a[k])) for k in ("phih_grid", "phihe_grid")}
    print("cells whose bits depend on planes first / last:", differ)
    assert differ["phih_grid"] > 0 and differ["phihe_grid"] > 0
    assert np.allclose(after["phih_grid"], mix_a["phih_grid"], rtol=1e-14, atol=0.0)


def test_a_callers_share(pkg, orc, otables, case_a):
    """The deal: share_of hands out 1..NumSrc + nplane by (first, stride); two callers' grids add up to the whole pass to
    rounding, and each is the composition over its own share."""
    assert mx.share_of(3, 2, 1, 2) == ([1, 3], [2]) and mx.share_of(3, 2, 2, 2) == ([2], [1])
    assert mx.share_of(4, 2, 1, 1) == ([1, 2, 3, 4], [1, 2]) and mx.share_of(0, 3, 2, 2) == ([], [2])
    whole = mx.compose(pkg, orc, otables, case_a, mx.PLANES_A, "mix_a", with_maps=False)
    one = mx.compose(pkg, orc, otables, case_a, mx.PLANES_A, "mix_a", first=1, stride=2, with_maps=False)
    two = mx.compose(pkg, orc, otables, case_a, mx.PLANES_A, "mix_a", first=2, stride=2, with_maps=False)
    assert (one["sources"], one["planes"], two["sources"], two["planes"]) == ([1, 3], [1], [2, 4], [2])
    assert one["sum_nbox"] + two["sum_nbox"] == whole["sum_nbox"]
    assert np.allclose(one["phih_grid"] + two["phih_grid"], whole["phih_grid"], rtol=1e-14, atol=0.0)


def test_the_fog_grid_maps_are_face_loss_references(pkg, orc, otables, case_a):
    """point_maps_fog_grid with a grid that holds one value everywhere equals face_loss_reference.expected with that scalar.
    With a random grid every fogged column it forms is held, inside the function, to the oracle's outgoing column of that cell
    (the oracle indexes the grid itself): that passes, and no longer does when the grid is handed over transposed."""
    lls = float(np.float32(2.0e16))
    grid = np.full(11 ** 3, lls, dtype=np.float32)
    _, want = fl.expected(pkg, orc, otables, case_a, "mix_a", sources=[0, 2], coldensh_lls=lls)
    for ns, ref in zip((0, 2), want):
        got = mx.point_maps_fog_grid(pkg, orc, otables, case_a, ns, grid)
        assert sorted(got) == sorted(ref) == [4, 5]
        assert all(np.array_equal(got[f], ref[f]) for f in ref) and any(ref[f].any() for f in ref)
    rough = (10.0 ** np.random.default_rng(7).uniform(15.5, 17, 11 ** 3)).astype(np.float32)
    for ns in (0, 3):
        got = mx.point_maps_fog_grid(pkg, orc, otables, case_a, ns, rough)
        assert all(got[f].any() and not np.array_equal(got[f], want[0][f]) for f in got)
    real = mx.embed_lls
    try:                        # the oracle keeps the grid as it is, the restatement reads a transposed one: the check inside fires
        mx.embed_lls = lambda case, grid, seed=99: real(case, rough, seed)
        with pytest.raises(AssertionError):
            mx.point_maps_fog_grid(pkg, orc, otables, case_a, 3, rough.reshape(11, 11, 11).transpose(0, 2, 1).copy().reshape(-1))
    finally:
        mx.embed_lls = real


# -- the product's host harnesses, adding into one array in plane order -------------------------------------------------------
def harness_fold(libs, case, planes):
    """Every plane through the harness that runs its kind (plane / oblique / flux), all adding into the same rate array, the
    way the device kernels add into the rate grids; per plane the exit columns and the terms."""
    ph_, ob_, fx_ = libs
    ndens, xh, xhe, _ = case.region
    n = ndens.size
    rates = np.zeros(4 * n)
    mesh, dr, per = (C.c_int * 3)(*case.n), (C.c_double * 3)(*case.dr), (C.c_int * 3)(*[int(b) for b in case.periodic])
    per_plane = []
    for pl in planes:
        face = pr.face_cells(case.n, pl["axis"])
        exit3, terms, cin, cflux, fexit = np.zeros(3 * face), np.zeros(face), np.zeros(n), np.zeros(3 * n), np.zeros(3 * face)
        tilted, mapped = mx.plane_kind(pl)
        entry = None if pl.get("entry") is None else _p(np.ascontiguousarray(pl["entry"], dtype=np.float64))
        tilt = (C.c_double * 2)(*(pl["tilt"] if tilted else (0.0, 0.0)))
        common = (mesh, dr, C.c_double(case.vol), _p(ndens), _p(xh), _p(xhe), pl["axis"], pl["from_high"])
        if mapped:
            fmap = np.ascontiguousarray(pl["fmap"], dtype=np.float64).reshape(-1)
            rc = fx_.fx_march(*common, _p(fmap), tilt, per, int(case.heat), 0, C.c_double(0.0), None, entry, _p(rates), _p(exit3), _p(terms),
                              _p(cin), _p(cflux), _p(fexit))
        elif tilted:
            rc = ob_.ob_march(*common, C.c_double(pl["normflux"]), tilt, per, int(case.heat), 0, C.c_double(0.0), None, entry, _p(rates),
                              _p(exit3), _p(terms), _p(cin))
        else:
            rc = ph_.ph_march(*common, C.c_double(pl["normflux"]), int(case.heat), 0, C.c_double(0.0), None, entry, _p(rates), _p(exit3),
                              _p(terms))
        assert rc == 0, (rc, pl["axis"])
        per_plane.append(dict(exit=exit3, terms=terms, exit_flux=fexit))
    return dict(phih_grid=rates[:n], phihe_grid=rates[n:3 * n], phiheat=rates[3 * n:]), per_plane


@pytest.mark.parametrize("heat", [False, True])
@pytest.mark.parametrize("tilted,mapped", [((2, 4), (3, 4)), ((3,), (2,))])
def test_the_host_harnesses_folded_in_plane_order(pkg, orc, otables, ph, obl, fx, tilted, mapped, heat):  # noqa: F811
    """Case c's four planes -- plain, tilted, mapped, tilted and mapped, through four faces of (11,11,24) -- and the same list
    with only the third tilted and only the second mapped: the product's functions, adding in plane order, give the composed
    plane part bit for bit; exit columns, exit flux and terms per plane.  Planes 2 and 3 have entry columns."""
    case = mx.make_case(pkg, "xy", np.zeros((0, 3)), np.zeros(0), heat=heat)
    planes = mx.planes_c(case, tilted, mapped)
    assert [p.get("entry") is not None for p in planes] == [False, True, True, False]
    assert [mx.plane_kind(p) for p in planes] == [(k in tilted, k in mapped) for k in (1, 2, 3, 4)]
    mix = mx.compose(pkg, orc, otables, case, planes, "harness", with_maps=False)
    got, per_plane = harness_fold((ph, obl, fx), case, planes)
    for k in GRIDS:
        assert np.array_equal(got[k], mix[k]), (k, int(np.count_nonzero(got[k] != mix[k])))
    assert bool(mix["phiheat"].any()) == heat
    for p, one in enumerate(per_plane, start=1):
        ref = mix["plane"][p]
        assert np.array_equal(one["exit"], ref["exit"]) and np.array_equal(one["terms"], ref["terms"]), p
        assert math.fsum(one["terms"]) == ref["loss"] and ref["loss"] > 0
        if p in mapped:
            assert np.array_equal(one["exit_flux"], ref["exit_flux"]), p
    # the fold is not the sum of any two orders by accident: the four planes overlap in every cell that all of them light
    lit = np.ones(mix["phih_grid"].size, dtype=bool)
    for p in (1, 2, 3, 4):
        lit &= mix["plane"][p]["phih_grid"] > 0
    assert lit.any()


# -- the generator of the random cases ------------------------------------------------------------------------------------------
def test_the_random_cases_of_the_default_seed(pkg, orc, otables3):
    """tests/test_gpu_plane_mix.py's generator with its default seed and count: at most a quarter of the drawn cases are
    redrawn for the embedding, every kept case has its tilts within one cell per layer, and the list is not lopsided."""
    import test_gpu_plane_mix as gm
    cases, redrawn = gm.random_cases(pkg, orc, otables3, gm.DEFAULT_CASES, gm.DEFAULT_SEED)
    print("kept", len(cases), "redrawn", redrawn)
    assert len(cases) == gm.DEFAULT_CASES and 4 * redrawn <= len(cases) + redrawn
    assert {c["mask"] for c in cases} >= {"z", "xy"} and max(len(c["planes"]) for c in cases) >= 3
    assert any(mx.plane_kind(p)[0] for c in cases for p in c["planes"]) and any(mx.plane_kind(p)[1] for c in cases for p in c["planes"])
    assert any(len(c["srcpos"]) == 0 for c in cases) or any(len(c["srcpos"]) >= 3 for c in cases)


def test_ionised_gas_runs_every_source_to_its_reach(pkg, orc, otables):
    """Case j: the oracle never stops early on the embedding (three rounds per source, 12 in all), the product's rounds are
    case.expected_rounds() = 11, and the composition carries both."""
    case = mx.case_j(pkg)
    mix = mx.compose(pkg, orc, otables, case, mx.PLANES_J, "mix_j", with_maps=False)
    assert mix["nbox"] == [3, 3, 3, 3] and all(mix["same_cells"]) and mix["oracle_sum_nbox"] == 12
    assert mix["sum_nbox"] == case.expected_rounds() == 11
