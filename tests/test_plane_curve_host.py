"""Plane light curves (c2r_set_plane_curve) on the CPU: the product's rule header (csrc/c2ray_pcurve.hpp) and the plane
headers compiled for the host (tests/plane_curve_harness.cpp) and marched over whole meshes the way the device kernels do,
against the Python reference (tests/plane_curve_reference.py): the factor of every layer, every rate grid, the incoming HI
columns, the exit columns, the exit flux and every line's loss term bit for bit.  Then the identities the header states, on
the reference and on the harness alike, and what the compiler made of the new kernels.
"""
import ctypes as C
import math
import os
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import flux_reference as fr
import oblique_reference as obr
import plane_curve_reference as pcr
import plane_reference as pr
from code_object import READELF, kernel_notes
from test_flux_reference_host import make_map, otables3  # noqa: F401  (otables3 is a fixture)
from test_oblique_reference_host import make_slab

ROOT = Path(__file__).resolve().parent.parent
OPEN = (False, False, False)
dp = C.POINTER(C.c_double)
KEYS = ("phih_grid", "phihe_grid", "phiheat", "cin_HI", "exit", "terms", "exit_flux", "factors")
RATES = ("phih_grid", "phihe_grid", "phiheat")
CXX = ["g++", "-O2", "-ffp-contract=off", "-mfma", "-std=c++17"]
TILT = (0.4, -0.7)
FLUX = 4.0e5


def _p(a):
    return a.ctypes.data_as(dp)


@pytest.fixture(scope="module")
def pc(pkg, gold):
    so = ROOT / "tests" / "_plane_curve_harness.so"
    srcs = [ROOT / "tests" / n for n in ("plane_curve_harness.cpp", "flux_harness.cpp", "plane_harness.cpp")]
    hdrs = list((ROOT / "c2-ray3dm1d_helium_amd" / "csrc").glob("*.hpp"))
    if not so.exists() or so.stat().st_mtime < max(p.stat().st_mtime for p in srcs + hdrs):
        r = subprocess.run(CXX + ["-fPIC", "-shared", "-o", str(so), str(srcs[0])], capture_output=True, text=True)
        if r.returncode != 0:
            pytest.fail("tests/plane_curve_harness.cpp does not compile against csrc/c2ray_pcurve.hpp:\n" + r.stderr[-2000:])
    lib = C.CDLL(str(so))
    t = pkg.RadiationTables.load()
    keep = [t.fvec[k] for k in pkg.evolve.FVEC_ORDER]
    fv = (dp * 12)(*[_p(a) for a in keep])
    lib.ph_set_tables(_p(t.photo_thick), _p(t.photo_thin), _p(t.heat_thick), _p(t.heat_thin), _p(t.sigma_HI), _p(t.sigma_HeI),
                      _p(t.sigma_HeII), fv, C.c_int(t.bb_upper))
    z = gold("rad_tables_pl_qpl.npz")
    seds = []
    for idx, pre in ((1, "pl_"), (2, "qpl_")):
        a = [np.ascontiguousarray(z[pre + k]) for k in ("photo_thick", "photo_thin", "heat_thick", "heat_thin")]
        lib.fx_set_sed(idx, *[_p(x) for x in a], C.c_int(int(z[pre + "limits"][0])), C.c_int(int(z[pre + "limits"][1])))
        seds.append(a)
    lib._keep = (t, keep, seds)
    return lib


def harness_factors(pc, curve, path, na):
    depths, factors, layer0, depth0 = pcr.unpack(curve)
    d, f, out = np.array(list(depths) + [0.0]), np.array(factors, dtype=np.float64), np.zeros(na)
    pc.pc_layer_factors(len(depths), _p(d), _p(f), layer0, C.c_double(depth0), C.c_double(path), na, _p(out))
    return out


def harness_march(pc, slab, mesh, axis, from_high, normflux=None, flux_map=None, curve=None, tilt=None, periodic=OPEN, heat=False, entry=None):
    (ndens, xh_av, xhe_av), dr, vol = slab
    n = ndens.size
    face = pr.face_cells(mesh, axis)
    rates, exit3, terms, cin = np.zeros(4 * n), np.zeros(3 * face), np.zeros(face), np.zeros(n)
    cflux, fexit, fac = np.zeros(3 * n), np.zeros(3 * face), np.zeros(mesh[axis])
    nf = fmap = None
    if flux_map is not None:
        fmap = np.ascontiguousarray(flux_map, dtype=np.float64).reshape(-1)
    else:
        nf = np.array((list(np.atleast_1d(normflux).astype(float)) + [0.0, 0.0])[:3])
    depths, factors, layer0, depth0 = pcr.unpack(curve)
    d, f = np.array(list(depths) + [0.0]), np.array(factors, dtype=np.float64)
    rc = pc.pc_march((C.c_int * 3)(*mesh), (C.c_double * 3)(*dr), C.c_double(vol), _p(ndens), _p(xh_av), _p(xhe_av), axis, from_high,
                     None if nf is None else _p(nf), None if fmap is None else _p(fmap), len(depths), _p(d), _p(f), layer0, C.c_double(depth0),
                     (C.c_double * 2)(*(tilt or (0.0, 0.0))), (C.c_int * 3)(*[int(b) for b in periodic]), int(heat), 0, C.c_double(0.0), None,
                     None if entry is None else _p(np.ascontiguousarray(entry)), _p(rates), _p(exit3), _p(terms), _p(cin), _p(cflux), _p(fexit),
                     _p(fac))
    assert rc == 0, f"pc_march returned {rc}"
    return dict(phih_grid=rates[:n], phihe_grid=rates[n:3 * n], phiheat=rates[3 * n:], exit=exit3, terms=terms, cin_HI=cin, exit_flux=fexit,
                factors=fac, loss=math.fsum(terms))


def both(pc, orc, otables, slab, mesh, axis, from_high, **kw):
    """The reference and the harness for one case, held to each other bit for bit: (reference, harness)."""
    (ndens, xh_av, xhe_av), dr, vol = slab
    ref = pcr.curve_pass(orc, otables, mesh, dr, vol, ndens, xh_av, xhe_av, axis, from_high, **kw)
    got = harness_march(pc, slab, mesh, axis, from_high, **kw)
    for k in KEYS:
        assert np.array_equal(got[k], ref[k]), (k, int(np.count_nonzero(got[k] != ref[k])))
    assert got["loss"] == ref["loss"]
    return ref, got


def gap_curve(dr, axis):
    """The issue's dark gap with light beyond it: {3, {1.2, 2.6, 4.1} * dr[axis], {1, 0.3, 0, 0.5}}."""
    return ([1.2 * dr[axis], 2.6 * dr[axis], 4.1 * dr[axis]], [1.0, 0.3, 0.0, 0.5])


def layer_mask(mesh, axis, from_high, layers):
    """Boolean over mesh cells: the cell lies in one of `layers` (travel order)."""
    cells = pr.column_cells(mesh, axis, from_high)
    mask = np.zeros(int(np.prod(mesh)), dtype=bool)
    mask[cells[:, list(layers)].reshape(-1)] = True
    return mask


# -- 1: the factor of every layer ----------------------------------------------------------------------------------------
def test_1_layer_factors_of_seeded_random_curves(pc):
    """Seeded random curves of 0..8 steps on meshes of 1..9 layers, with layer0 > 0 and depth0 > 0: the harness' factors are the
    Python rule's."""
    rng = np.random.default_rng(20261020)
    seen = set()
    for _ in range(300):
        nstep = int(rng.integers(0, 9))
        na, path = int(rng.integers(1, 10)), float(rng.uniform(0.5, 2.0)) * 1.0e22
        layer0 = int(rng.integers(0, 5))
        depth0 = float(rng.choice([0.0, rng.uniform(0.0, 3.0) * path]))
        depths = list(np.cumsum(rng.uniform(0.05, 2.5, nstep)) * path)
        factors = [float(rng.choice([0.0, 1.0, 0.5, rng.uniform(0.0, 3.0)])) for _ in range(nstep + 1)]
        if nstep == 0 and factors[0] == 0.0:
            factors[0] = 0.75
        curve = (depths, factors, layer0, depth0)
        want = np.array([pcr.layer_factor(curve, m, path) for m in range(na)])
        assert np.array_equal(harness_factors(pc, curve, path, na), want), curve
        seen.add((nstep, layer0 > 0, depth0 > 0))
    assert {s[0] for s in seen} == set(range(9)) and any(s[1] and s[2] for s in seen)


def test_1_a_centre_on_a_depth_belongs_to_the_nearer_shell(pc):
    """path = 1.0, depth = {2.5}: layer 2's centre is exactly 2.5 and keeps factor[0]; with layer0 = 1 it is layer 1's."""
    assert pcr.layer_depth(0.0, 0, 2, 1.0) == 2.5
    for layer0, want in ((0, [7.0, 7.0, 7.0, 3.0, 3.0]), (1, [7.0, 7.0, 3.0, 3.0, 3.0])):
        curve = ([2.5], [7.0, 3.0], layer0, 0.0)
        assert [pcr.layer_factor(curve, m, 1.0) for m in range(5)] == want
        assert list(harness_factors(pc, curve, 1.0, 5)) == want
    # depth0 moves the centre off the step by one unit in the last place: the farther shell
    curve = ([2.5], [7.0, 3.0], 0, 2.0 ** -51)
    assert list(harness_factors(pc, curve, 1.0, 4)) == [7.0, 7.0, 3.0, 3.0] == [pcr.layer_factor(curve, m, 1.0) for m in range(4)]


def test_1_no_step_and_eight_steps(pc):
    """nstep = 0: factor[0] everywhere; nstep = 8: every one of the nine shells is reached."""
    assert list(harness_factors(pc, ([], [0.625]), 1.0e22, 9)) == [0.625] * 9
    curve = ([float(k + 1) for k in range(8)], [float(10 + k) for k in range(9)])
    want = [float(10 + m) for m in range(9)]                # centre m + 0.5 lies behind m steps
    assert list(harness_factors(pc, curve, 1.0, 9)) == want == [pcr.layer_factor(curve, m, 1.0) for m in range(9)]


# -- 2: the reference's anchors -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def slab765(pkg):
    return make_slab(pkg, (7, 6, 5), 2026, (1.0, 1.3, 0.8))


def test_2_all_ones_is_the_uncurved_reference(orc, otables, slab765):
    """All factors 1.0 on (7,6,5): curve_pass equals plane_pass (uniform), oblique_pass (tilted) and flux_pass (mapped, normal and
    tilted) bit for bit."""
    mesh = (7, 6, 5)
    (ndens, xh_av, xhe_av), dr, vol = slab765
    ones = ([1.0 * dr[2], 3.0 * dr[2]], [1.0, 1.0, 1.0], 2, 0.3 * dr[2])
    args = (orc, otables, mesh, dr, vol, ndens, xh_av, xhe_av, 2, 0)
    fmap = make_map(pr.face_cells(mesh, 2), 1)
    pairs = [(pr.plane_pass(*args, FLUX), pcr.curve_pass(*args, normflux=FLUX, curve=ones)),
             (obr.oblique_pass(*args, FLUX, TILT, periodic=(True, False, False)),
              pcr.curve_pass(*args, normflux=FLUX, curve=ones, tilt=TILT, periodic=(True, False, False))),
             (fr.flux_pass(*args, fmap), pcr.curve_pass(*args, flux_map=fmap, curve=ones)),
             (fr.flux_pass(*args, fmap, tilt=TILT), pcr.curve_pass(*args, flux_map=fmap, curve=ones, tilt=TILT))]
    for old, new in pairs:
        for k in old:
            assert np.array_equal(old[k], new[k]), k
        assert new["phih_grid"].any() and np.all(new["factors"] == 1.0)


# -- 3: the harness march against the reference -------------------------------------------------------------------------
@pytest.mark.parametrize("axis,from_high", [(0, 1), (1, 0), (2, 0)])
def test_3_dark_gap_uniform(pc, orc, otables, slab765, axis, from_high):
    """(7,6,5), normal incidence through three faces, uniform flux, the dark-gap curve: unlit layers hold exactly 0, the layers
    behind the gap are lit again."""
    mesh, dr = (7, 6, 5), slab765[1]
    ref, _ = both(pc, orc, otables, slab765, mesh, axis, from_high, normflux=FLUX, curve=gap_curve(dr, axis))
    want = [1.0, 0.3, 0.3, 0.0, 0.5, 0.5, 0.5][:mesh[axis]]              # centres 0.5, 1.5, 2.5, 3.5, 4.5, 5.5, 6.5 cells
    assert list(ref["factors"]) == want
    dark = layer_mask(mesh, axis, from_high, [3])
    for k in RATES:
        assert not ref[k].reshape(-1, dark.size)[:, dark].any(), k
    assert np.all(ref["phih_grid"][~dark] > 0) and ref["terms"].any()


def test_3_dark_gap_with_a_map(pc, orc, otables, slab765):
    mesh, dr = (7, 6, 5), slab765[1]
    fmap = make_map(pr.face_cells(mesh, 0), 1)
    ref, _ = both(pc, orc, otables, slab765, mesh, 0, 1, flux_map=fmap, curve=gap_curve(dr, 0))
    assert np.array_equal(ref["exit_flux"], fmap.reshape(-1)) and not ref["terms"][fmap[0] == 0.0].any() and ref["terms"].any()


def test_3_tilted_heating_three_sed_maps(pc, orc, otables3, pkg):
    """(6,5,4), tilted, heating, a map per SED, a curve with a non-power-of-two factor and an unlit layer, layer0 and depth0."""
    mesh = (6, 5, 4)
    slab = make_slab(pkg, mesh, 2028, (1.0, 1.3, 0.8))
    fmap = make_map(pr.face_cells(mesh, 0), 3, seds=3)
    fmap[1, 7] = 0.0
    path = pcr.plane_path(slab[1], 0, (0.0, 0.55))
    curve = ([2.2 * path, 3.1 * path, 4.4 * path], [0.7, 1.3, 0.0, 0.45], 1, 0.5 * path)
    ref, _ = both(pc, orc, otables3, slab, mesh, 0, 1, flux_map=fmap, curve=curve, tilt=(0.0, 0.55), heat=True)
    assert list(ref["factors"]) == [0.7, 1.3, 0.0, 0.45, 0.45, 0.45] and np.any(ref["phiheat"] > 0)  # centres 2, 3, .. 7 paths deep


# -- 4: identities ---------------------------------------------------------------------------------------------------------
def test_4_step_to_zero_is_a_depth_horizon(pc, orc, otables, slab765):
    """{1, {D}, {1, 0}} with D = 3 layers: the first three layers have the uncurved bits, the last two exactly zero, loss 0.0."""
    mesh, dr = (7, 6, 5), slab765[1]
    (ndens, xh_av, xhe_av), _, vol = slab765
    plain = pr.plane_pass(orc, otables, mesh, dr, vol, ndens, xh_av, xhe_av, 2, 1, FLUX)
    for res in both(pc, orc, otables, slab765, mesh, 2, 1, normflux=FLUX, curve=([3.0 * dr[2]], [1.0, 0.0])):
        assert list(res["factors"]) == [1.0, 1.0, 1.0, 0.0, 0.0]
        near = layer_mask(mesh, 2, 1, [0, 1, 2])
        for k in RATES:
            g, p = res[k].reshape(-1, near.size), plain[k].reshape(-1, near.size)
            assert np.array_equal(g[:, near], p[:, near]) and not g[:, ~near].any(), k
        assert not res["terms"].any() and res["loss"] == 0.0
        assert np.array_equal(res["exit"], plain["exit"]) and np.array_equal(res["cin_HI"], plain["cin_HI"])


def test_4_a_power_of_two_scales_exactly(pc, orc, otables, slab765):
    """factor 2^-3 everywhere behind the first layer: rates and loss terms are the uncurved ones times 0.125, exactly."""
    mesh, dr = (7, 6, 5), slab765[1]
    (ndens, xh_av, xhe_av), _, vol = slab765
    fmap = make_map(pr.face_cells(mesh, 2), 1)
    plain = fr.flux_pass(orc, otables, mesh, dr, vol, ndens, xh_av, xhe_av, 2, 0, fmap)
    for res in both(pc, orc, otables, slab765, mesh, 2, 0, flux_map=fmap, curve=([1.0 * dr[2]], [1.0, 0.125])):
        first = layer_mask(mesh, 2, 0, [0])
        for k in RATES[:2]:
            g, p = res[k].reshape(-1, first.size), plain[k].reshape(-1, first.size)
            assert np.array_equal(g[:, first], p[:, first]) and np.array_equal(g[:, ~first], 0.125 * p[:, ~first]) and p.any(), k
        assert np.array_equal(res["terms"], 0.125 * plain["terms"]) and res["terms"].any()


def test_4_two_slabs_equal_one_mesh(pc, orc, otables, pkg):
    """(7,6,3) into (7,6,2) with layer0 = 3 against (7,6,5), tilted, with a map: the exit columns and the UNSCALED exit flux are
    handed on; rates of both parts, the final exit columns, the exit flux and every loss term bit for bit."""
    mesh = (7, 6, 5)
    slab = make_slab(pkg, mesh, 2029, (1.0, 1.3, 0.8))
    (ndens, xh_av, xhe_av), dr, vol = slab
    fmap = make_map(pr.face_cells(mesh, 2), 4)
    path = pcr.plane_path(dr, 2, TILT)
    depths, factors, depth0 = [1.5 * path, 3.7 * path, 4.5 * path], [1.0, 0.6, 0.0, 1.7], 0.25 * path
    per = (True, False, False)

    def part(lo, hi):
        cut = lambda a, comps: a.reshape(comps, 5, 6, 7)[:, lo:hi].reshape(-1).copy()
        return (cut(ndens, 1), cut(xh_av, 2), cut(xhe_av, 3)), dr, vol
    whole = both(pc, orc, otables, slab, mesh, 2, 0, flux_map=fmap, curve=(depths, factors, 0, depth0), tilt=TILT, periodic=per)
    lower = both(pc, orc, otables, part(0, 3), (7, 6, 3), 2, 0, flux_map=fmap, curve=(depths, factors, 0, depth0), tilt=TILT, periodic=per)
    for big, low in zip(whole, lower):
        up_ref, up = both(pc, orc, otables, part(3, 5), (7, 6, 2), 2, 0, flux_map=low["exit_flux"], curve=(depths, factors, 3, depth0), tilt=TILT,
                          periodic=per, entry=low["exit"])
        assert list(big["factors"]) == list(low["factors"]) + list(up["factors"]) == [1.0, 0.6, 0.6, 0.0, 1.7]
        for k in RATES[:2]:
            b = big[k].reshape(-1, 5, 6, 7)
            assert np.array_equal(b[:, :3].reshape(-1), low[k]) and np.array_equal(b[:, 3:].reshape(-1), up[k]), k
        for k in ("exit", "exit_flux", "terms"):
            assert np.array_equal(big[k], up[k]), k
        assert big["loss"] == up["loss"] > 0 and not np.array_equal(low["exit_flux"], fmap.reshape(-1))


# -- 5: the code object ----------------------------------------------------------------------------------------------------
def test_5_curved_kernels_in_the_code_object(pkg):
    """Every k_pcurve_ kernel exists -- 12 rates and 8 exit instantiations; the isothermal rates kernels and every exit kernel have
    no private segment; the heating ones are printed next to their k_plane_rates twins."""
    if not Path(READELF).exists():
        pytest.skip("llvm-readelf not present")
    notes = kernel_notes(pkg.build())
    mine = {n: v for n, v in notes.items() if "k_pcurve_" in n}
    rates = [n for n in mine if re.search(r"14k_pcurve_ratesILb[01]ELb[01]ELNS_9PlaneFluxE[012]EE", n)]
    exits = [n for n in mine if re.search(r"13k_pcurve_exitILb[01]ELb[01]ELb[01]EE", n)]
    assert len(rates) == 12 and len(exits) == 8 and len(mine) == 20, sorted(mine)
    assert not [n for n in mine if "k_plane_" in n or "k_loss" in n]
    cold = exits + [n for n in rates if "k_pcurve_ratesILb0E" in n]
    assert len(cold) == 8 + 6 and {n: mine[n]["private_segment"] for n in cold if mine[n]["private_segment"]} == {}
    for n in sorted(rates):
        if "k_pcurve_ratesILb1E" in n:
            inst = re.search(r"k_pcurve_rates(I.*?PlaneFluxE[012]EE)", n).group(1)
            twin = [v for t, v in notes.items() if "k_plane_rates" + inst in t]
            assert len(twin) == 1, inst
            print(inst, "curved", mine[n], "twin", twin[0])


# -- 6: the harness alone under host sanitizers ---------------------------------------------------------------------------
def test_6_the_harness_alone_is_clean_under_host_sanitizers(tmp_path):
    """tests/plane_curve_harness.cpp as a stand-alone program (-DPCURVE_MAIN) under AddressSanitizer and UBSan: every cell's layer
    for every face, and the table reads of curves of 0, 3 and 8 steps."""
    exe = tmp_path / "pcurve_main"
    r = subprocess.run(CXX + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DPCURVE_MAIN", "-o", str(exe),
                              str(ROOT / "tests" / "plane_curve_harness.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    print(r.stdout, r.stderr[-2000:])
    assert r.returncode == 0 and "cells missed or repeated: 0" in r.stdout
