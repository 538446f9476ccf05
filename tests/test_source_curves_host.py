"""Source light curves (c2r_set_source_curves) on the CPU.

1. The functions of csrc/c2ray_curve.hpp -- the code the kernels run per lane -- compiled for the host
   (tests/curve_harness.cpp) against the NumPy restatement of tests/curve_reference.py, with == on every offset of a
   25 x 25 x 25 cube around the source (|o| <= 12):
     * cubic cells whose dr is a power of two, radii 3 dr and 5 dr: every product is exact, so integer arithmetic says which
       shell a cell is in, and the Pythagorean cells on a radius fall in the inner shell;
     * cells with dr = (d, 1.25 d, 0.75 d), and a radius whose square IS a cell's d2;
     * nstep = 0 and nstep = 8; a factor of 0 in a middle shell;
     * a cone, a horizon and a curve through cut_flux against the product of the three NumPy restatements.
2. The reference against the oracle at 16^3: all factors 1.0 is beam_reference.compose; a power-of-two factor scales the
   oracle's grids and loss exactly (the premise behind f*term), 0.3 does not.
3. The bindings, and the notes of the gfx950 code object against profiles/source_curves_resources.json.
"""
import ctypes as C
import json
import subprocess
from pathlib import Path

import numpy as np
import pytest

import beam_reference as br
import curve_reference as cr
import horizon_reference as hr
import mix_reference as mr
from code_object import READELF, kernel_notes
from test_source_beams_host import two_source_case
from test_source_horizons_host import HALF, P2, D, BOX, cube_offsets, at, signed_permutations

ROOT = Path(__file__).resolve().parent.parent
INF = float("inf")


@pytest.fixture(scope="module")
def ch():
    so = ROOT / "tests" / "_curve_harness.so"
    src = ROOT / "tests" / "curve_harness.cpp"
    hdrs = list((ROOT / "c2-ray3dm1d_helium_amd" / "csrc").glob("*.hpp"))
    if not so.exists() or so.stat().st_mtime < max(p.stat().st_mtime for p in [src] + hdrs):
        r = subprocess.run(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-std=c++17", "-o", str(so), str(src)],
                           capture_output=True, text=True)
        if r.returncode != 0:
            pytest.fail("tests/curve_harness.cpp does not compile against csrc/c2ray_curve.hpp:\n" + r.stderr[-2000:])
    lib = C.CDLL(str(so))
    dp = C.POINTER(C.c_double)
    lib.ch_curve_R2.restype = C.c_double
    lib.ch_curve_R2.argtypes = [C.c_double]
    lib.ch_factor_cube.restype = None
    lib.ch_factor_cube.argtypes = [C.c_int, dp, dp, dp, C.c_int, dp]
    lib.ch_cut_cube.restype = None
    lib.ch_cut_cube.argtypes = [C.c_int, dp, C.c_double, C.c_double, C.c_int, dp, dp, dp, C.c_int, C.POINTER(C.c_ubyte), dp]
    return lib


def _tables(curve):
    radii, factors = curve
    r = (C.c_double * cr.MAX_STEPS)(*radii)
    f = (C.c_double * (cr.MAX_STEPS + 1))(*factors)
    return len(radii), r, f


def header_factor(ch, curve, dr):
    w = 2 * HALF + 1
    out = (C.c_double * (w * w * w))()
    n, r, f = _tables(curve)
    ch.ch_factor_cube(n, r, f, (C.c_double * 3)(*dr), HALF, out)
    return np.frombuffer(out, dtype=np.float64).reshape(w, w, w).copy()


def header_cut(ch, beam, hradius, curve, dr):
    kind, axis, cos_half = (0, (0.0, 0.0, 0.0), 0.0) if beam is None else beam
    w = 2 * HALF + 1
    lit, out = (C.c_ubyte * (w * w * w))(), (C.c_double * (w * w * w))()
    n, r, f = _tables(curve)
    ch.ch_cut_cube(int(kind), (C.c_double * 3)(*axis), float(cos_half), float(hradius), n, r, f, (C.c_double * 3)(*dr), HALF, lit, out)
    return np.frombuffer(lit, dtype=np.uint8).reshape(w, w, w).astype(bool), np.frombuffer(out, dtype=np.float64).reshape(w, w, w).copy()


def check(ch, curve, dr):
    """The header's two routes against the restatement, == on every cell; returns (the factor cube, the shell cube)."""
    di, dj, dk = cube_offsets()
    got, want = header_factor(ch, curve, dr), cr.factor_offsets(curve, dr, di, dj, dk)
    shell = cr.shell_offsets(curve, dr, di, dj, dk)
    print("radii", curve[0], "dr", dr, "cells per shell", np.bincount(shell.reshape(-1)).tolist(), "differ", int(np.count_nonzero(got != want)))
    for r in curve[0]:
        assert ch.ch_curve_R2(float(r)) == float(cr.curve_R2(r))
    assert np.array_equal(got, want), curve
    lit, f = header_cut(ch, None, INF, curve, dr)
    assert np.array_equal(lit, want != 0.0) and np.array_equal(f, np.where(want != 0.0, want, 0.0)), curve
    assert shell[HALF, HALF, HALF] == 0 and got[HALF, HALF, HALF] == curve[1][0], "the source's own cell is shell 0"
    return got, shell


def test_cubic_power_of_two_cells_are_exact(ch):
    """dr = 2^81, radii 3 dr and 5 dr: the shell is the number of {9, 25} below di^2 + dj^2 + dk^2 in integers, and a cell exactly
    on a radius belongs to the inner shell."""
    dr = (P2, P2, P2)
    di, dj, dk = cube_offsets()
    r2 = di * di + dj * dj + dk * dk
    curve = ([3 * P2, 5 * P2], [1.0, 0.3, 2.5])
    f, shell = check(ch, curve, dr)
    assert np.array_equal(shell, (r2 > 9).astype(np.int64) + (r2 > 25))
    assert np.array_equal(f, np.where(r2 <= 9, 1.0, np.where(r2 <= 25, 0.3, 2.5)))
    for o in signed_permutations((1, 2, 2)) | signed_permutations((0, 0, 3)):      # exactly on the radius 3: inner
        assert f[o[2] + HALF, o[1] + HALF, o[0] + HALF] == 1.0, o
    for o in signed_permutations((3, 4, 0)) | signed_permutations((0, 0, 5)):      # exactly on the radius 5: the middle shell
        assert f[o[2] + HALF, o[1] + HALF, o[0] + HALF] == 0.3, o
    for o in signed_permutations((3, 4, 1)) | signed_permutations((0, 0, 6)):
        assert f[o[2] + HALF, o[1] + HALF, o[0] + HALF] == 2.5, o
    for o in signed_permutations((2, 2, 2)):
        assert f[o[2] + HALF, o[1] + HALF, o[0] + HALF] == 0.3, o


def test_cells_that_are_no_cubes(ch):
    """dr = (d, 1.25 d, 0.75 d): the shells follow physical lengths, and a cell whose d2 is R2 bit for bit is in the inner one."""
    di, dj, dk = cube_offsets()
    curve = ([3.3 * D, 6.1 * D], [2.0, 1.0, 0.25])
    f, shell = check(ch, curve, BOX)
    assert not np.array_equal(shell, ((di * di + dj * dj + dk * dk) > 3.3 ** 2).astype(np.int64) + ((di * di + dj * dj + dk * dk) > 6.1 ** 2))
    assert shell[HALF + 4, HALF, HALF] == 0 and shell[HALF, HALF + 3, HALF] == 1 and shell[HALF, HALF, HALF + 4] == 1     # 3 d, 3.75 d, 4 d
    # radius = dr2 * 4: its square is the d2 of (0, +-4, 0) -- (0 + ys*ys) + 0 -- exactly
    radius = BOX[1] * 4.0
    xs, ys, zs = BOX[0] * di.astype(np.float64), BOX[1] * dj.astype(np.float64), BOX[2] * dk.astype(np.float64)
    d2 = (xs * xs + ys * ys) + zs * zs
    assert radius * radius == d2[HALF, HALF + 4, HALF]
    f, shell = check(ch, ([radius], [1.0, 0.5]), BOX)
    assert f[HALF, HALF + 4, HALF] == 1.0 and f[HALF, HALF - 4, HALF] == 1.0 and f[HALF, HALF + 5, HALF] == 0.5
    assert f[HALF, HALF, HALF + 5] == 1.0 and f[HALF, HALF, HALF + 6] == 0.5
    inner = float(np.nextafter(radius, 0.0))
    f, _ = check(ch, ([inner], [1.0, 0.5]), BOX)
    assert f[HALF, HALF + 4, HALF] == 0.5


@pytest.mark.parametrize("cells", ["cubic", "box"])
def test_no_step_eight_steps_and_a_dark_middle_shell(ch, cells):
    dr = (P2, P2, P2) if cells == "cubic" else BOX
    d = dr[0]
    f, shell = check(ch, ([], [0.5]), dr)                                            # nstep = 0: one shell, everywhere
    assert np.all(f == 0.5) and not shell.any()
    radii = [1.5 * d, 2.5 * d, 4.0 * d, 5.5 * d, 7.0 * d, 9.0 * d, 11.0 * d, 14.0 * d]
    factors = [1.0, 0.25, 3.0 / 7.0, 2.0, 0.0, 1.9, 0.5, 4.0, 0.125]
    f, shell = check(ch, (radii, factors), dr)                                       # nstep = 8
    assert sorted(set(shell.reshape(-1).tolist())) == list(range(9))
    lit, ff = header_cut(ch, None, INF, (radii, factors), dr)
    assert np.array_equal(lit, shell != 4) and (shell == 4).sum() > 100               # the dark shell is unlit, nothing else is
    f, shell = check(ch, ([0.0], [0.0, 0.0]), dr)                                     # a source that has gone dark
    assert not f.any() and shell[HALF, HALF, HALF] == 0 and shell.sum() == shell.size - 1
    f, _ = check(ch, ([1e200], [1.0, 0.0]), dr)                                       # R2 overflows: nothing is beyond
    assert np.all(f == 1.0)


@pytest.mark.parametrize("cells", ["cubic", "box"])
def test_cone_horizon_and_curve_is_the_product_of_the_three(ch, cells):
    dr = (D, D, D) if cells == "cubic" else BOX
    di, dj, dk = cube_offsets()
    beams = [None, (br.CONE, (0.0, 0.0, 1.0), 0.7071067811865475), (br.BICONE, (1.0, 1.0, 0.0), 0.5),
             (br.CONE, (1.0, 2.0, -1.0), float(np.cos(np.radians(30.0))))]
    curve = ([2.5 * D, 4.5 * D, 8.0 * D], [1.0, 0.0, 0.3, 2.0])
    for beam in beams:
        for hradius in (0.0, 4.5 * D, 7.0 * D, 1e200, INF):
            lit, f = header_cut(ch, beam, hradius, curve, dr)
            want_f = cr.factor_offsets(curve, dr, di, dj, dk)
            want = hr.lit_offsets(beam, hradius, dr, di, dj, dk) & (want_f != 0.0)
            print(cells, beam, hradius, "lit", int(lit.sum()), "differ", int(np.count_nonzero(lit != want)))
            assert np.array_equal(lit, want) and np.array_equal(f, np.where(want, want_f, 0.0)), (beam, hradius)
            assert lit[HALF, HALF, HALF]
    lit, _ = header_cut(ch, beams[1], 7.0 * D, curve, dr)
    assert 0 < lit.sum() < hr.lit_offsets(beams[1], 7.0 * D, dr, di, dj, dk).sum()


# -- the reference against the oracle ----------------------------------------------------------------------------------------
def test_all_factors_one_is_the_beam_composition(pkg, orc, otables):
    case = two_source_case(pkg, heat=True)
    dr = float(case.dr[0])
    plain = br.compose(pkg, orc, otables, case, "host16_heat", [None, None])
    for curves in ([None, None], [([3.5 * dr, 6.5 * dr], [1.0, 1.0, 1.0]), None], [([], [1.0]), ([2.0 * dr], [1.0, 1.0])]):
        ref = cr.compose(pkg, orc, otables, case, "host16_heat", curves)
        for k in cr.GRIDS:
            assert np.array_equal(ref[k], plain[k]), (k, curves)
        assert all(nb == 1 for per in ref["nbox"] for nb in per)
    # a dark middle shell leaves source 2's grid alone there, and with a horizon the composition is horizon_reference's
    curves = [([3.5 * dr, 6.5 * dr], [1.0, 0.0, 1.0]), None]
    ref = cr.compose(pkg, orc, otables, case, "host16_heat", curves)
    dark = cr.shell_cells(case, 0, curves[0]) == 1
    alone2 = br.source_alone(pkg, orc, otables, case, "host16_heat", 2)[0]
    assert 0 < dark.sum() < dark.size
    for g in cr.GRIDS:
        m = np.tile(dark, ref[g].size // dark.size)
        assert np.array_equal(ref[g][m], (0.0 + alone2[g])[m]) and np.array_equal(ref[g][~m], plain[g][~m]), g
    step = cr.compose(pkg, orc, otables, case, "host16_heat", [([4.5 * dr], [1.0, 0.0]), None])
    hz = hr.compose(pkg, orc, otables, case, "host16_heat", [4.5 * dr, None])
    for g in cr.GRIDS:
        assert np.array_equal(step[g], hz[g]), g


@pytest.mark.parametrize("heat", [False, True])
def test_a_power_of_two_scales_the_oracle_exactly(pkg, orc, otables, heat):
    """The premise of the reference: a source's flux times 0.5 or 4 scales phih, phihe, phiheat and the loss exactly; times 0.3
    it does not, but stays within 1e-12 relative -- so a general factor needs the oracle's run at the rounded product."""
    case = two_source_case(pkg, heat=heat)
    key = "host16_heat" if heat else "host16_iso"
    base, nb, loss, _ = br.source_alone(pkg, orc, otables, case, key, 1)
    for f in (0.5, 4.0):
        grids, nb_f, loss_f, _ = cr.source_scaled(pkg, orc, otables, case, key, 1, f)
        assert nb_f == nb == 1 and loss_f == f * loss
        for g in cr.GRIDS:
            assert np.array_equal(grids[g], f * base[g]), (f, g)
    grids, nb_f, loss_f, _ = cr.source_scaled(pkg, orc, otables, case, key, 1, 0.3)
    worst = 0.0
    for g in cr.GRIDS:
        ref = 0.3 * base[g]
        nz = ref != 0.0
        if nz.any():
            worst = max(worst, float(np.max(np.abs(grids[g][nz] - ref[nz]) / np.abs(ref[nz]))))
    print("0.3: worst relative difference from 0.3*grid", worst, "grids equal", all(np.array_equal(grids[g], 0.3 * base[g]) for g in cr.GRIDS))
    assert 0.0 < worst < 1e-12


# -- the bindings and the code object ------------------------------------------------------------------------------------------
def test_bindings_have_the_two_calls(pkg):
    assert hasattr(pkg.HipEngine, "set_source_curves") and hasattr(pkg.HipEngine, "source_curve")
    assert "c2r_set_source_curves" in pkg._lib.SYMBOLS and "c2r_get_source_curve" in pkg._lib.SYMBOLS
    assert C.sizeof(pkg._lib.SourceCurve) == 8 + 8 * 8 + 9 * 8
    f = (ROOT / "c2-ray3dm1d_helium_amd" / "fortran" / "c2ray_hip_binding.f90").read_text()
    assert 'bind(C, name="c2r_set_source_curves")' in f and 'bind(C, name="c2r_get_source_curve")' in f
    assert "type, bind(C) :: c2r_source_curve" in f
    h = (ROOT / "include" / "c2ray_hip.h").read_text()
    assert "#define C2R_CURVE_MAX_STEPS 8" in h
    assert "int c2r_set_source_curves(c2r_ctx *ctx, int nsrc, const c2r_source_curve *curves);" in h
    assert "int c2r_get_source_curve(const c2r_ctx *ctx, int ns, c2r_source_curve *out);" in h


def test_rates_kernels_in_the_code_object(pkg):
    """profiles/source_curves_resources.json: every k_rates and k_rates_beam instantiation has the parent commit's figures
    ('before'), no k_rates_curve instantiation has a private segment (none of its k_rates_beam twins has one) or more than the
    128 vector registers of the four waves per SIMD its __launch_bounds__ asks for, and 'after' is what the library holds."""
    if not Path(READELF).exists():
        pytest.skip("llvm-readelf not present")
    notes = kernel_notes(pkg.build())
    curve = {n: v for n, v in notes.items() if "13k_rates_curveILb" in n}
    beam = {n: v for n, v in notes.items() if "12k_rates_beamILb" in n}
    plain = {n: v for n, v in notes.items() if "7k_ratesILb" in n}
    assert len(curve) == 8 and len(beam) == 8 and len(plain) == 8, sorted(notes)
    for n, v in sorted(curve.items()):
        twin = beam[n.replace("13k_rates_curveILb", "12k_rates_beamILb")]
        print(n[:50], v, "twin", twin)
        assert v["private_segment"] == 0 and twin["private_segment"] == 0 and v["vgpr"] + v["agpr"] <= 128, (n, v)
    rec = json.loads((ROOT / "profiles" / "source_curves_resources.json").read_text())
    keys = ("vgpr", "agpr", "sgpr", "private_segment", "lds")
    before = {v["mangled"]: {k: v[k] for k in keys} for v in rec["before"].values() if "k_rates" in v["mangled"]}
    after = {v["mangled"]: {k: v[k] for k in keys} for v in rec["after"].values() if "k_rates" in v["mangled"]}
    assert before == {**plain, **beam}, "k_rates and k_rates_beam are the parent's"
    assert after == {**plain, **beam, **curve}
