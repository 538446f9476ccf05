"""Horizon loss (c2r_enable_horizon_loss) on the CPU.

1. The rule of csrc/c2ray_rim.hpp -- the code k_horizon_rim runs per lane -- compiled for the host (tests/rim_harness.cpp)
   against the restatement of tests/rim_reference.py, which finds k* by scanning: == on k*, the face flag, the column's cell
   and w for every sheet column of a box; the decode against its inverse.
     * cubic cells, radius 0, 0.5, 1, 2.3, 3 (cells exactly on the sphere), 5 and 7.7 cells, in a box that contains the sphere;
     * dr = (1, 1.3, 0.7);
     * an asymmetric box (lo != -hi) smaller than the sphere on one side: its surface cells give no face;
     * a cone: beam-unlit columns have no face.
2. The tiling identity: for a box that contains the sphere and a radius >= 5 max(dr), |sum of w - 1| <= 1e-3.
3. The Python face_sum against the C++ face_sum of csrc/c2ray_face.hpp, == on random terms.
4. The bindings.
"""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import beam_reference as br
import rim_reference as rr

ROOT = Path(__file__).resolve().parent.parent
CUBIC = (1.0, 1.0, 1.0)
BOX = (1.0, 1.3, 0.7)
D = 2.3e24                                   # a cell size of the order the test grids have, no power of two
RADII = (0.0, 0.5, 1.0, 2.3, 3.0, 5.0, 7.7)
CONE = (br.CONE, (1.0, 2.0, -1.0), float(np.cos(np.radians(40.0))))


@pytest.fixture(scope="module")
def rh():
    so = ROOT / "tests" / "_rim_harness.so"
    src = ROOT / "tests" / "rim_harness.cpp"
    hdrs = list((ROOT / "c2-ray3dm1d_helium_amd" / "csrc").glob("*.hpp"))
    if not so.exists() or so.stat().st_mtime < max(p.stat().st_mtime for p in [src] + hdrs):
        r = subprocess.run(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-std=c++17", "-o", str(so), str(src)],
                           capture_output=True, text=True)
        if r.returncode != 0:
            pytest.fail("tests/rim_harness.cpp does not compile against csrc/c2ray_rim.hpp:\n" + r.stderr[-2000:])
    lib = C.CDLL(str(so))
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    lib.rh_total.restype = C.c_longlong
    lib.rh_total.argtypes = [ip, ip]
    lib.rh_columns.restype = C.c_int
    lib.rh_columns.argtypes = [C.c_int, dp, C.c_double, C.c_double, dp, ip, ip, ip, C.POINTER(C.c_ubyte), dp, ip, ip]
    lib.rh_face_sum.restype = C.c_double
    lib.rh_face_sum.argtypes = [dp, C.c_longlong]
    return lib


def header_columns(rh, radius, dr, lo, hi, beam=None):
    kind, axis, cos_half = (0, (0.0, 0.0, 0.0), 0.0) if beam is None else beam
    lo_a, hi_a = (C.c_int * 3)(*lo), (C.c_int * 3)(*hi)
    T = int(rh.rh_total(lo_a, hi_a))
    assert T == rr.total(lo, hi)
    kstar, cell, col = np.zeros(T, dtype=np.int32), np.zeros(3 * T, dtype=np.int32), np.zeros(3 * T, dtype=np.int32)
    face, w = np.zeros(T, dtype=np.uint8), np.zeros(T)
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    bad = rh.rh_columns(int(kind), (C.c_double * 3)(*axis), float(cos_half), float(radius), (C.c_double * 3)(*dr), lo_a, hi_a,
                        kstar.ctypes.data_as(ip), face.ctypes.data_as(C.POINTER(C.c_ubyte)), w.ctypes.data_as(dp),
                        cell.ctypes.data_as(ip), col.ctypes.data_as(ip))
    assert bad == 0, "rim_decode and rim_index disagree"
    return dict(kstar=kstar, face=face.astype(bool), w=w, cell=cell.reshape(-1, 3), col=col.reshape(-1, 3))


def check(rh, radius, dr, lo, hi, beam=None):
    """The header against the restatement, == on every column; returns the restatement's arrays."""
    got, want = header_columns(rh, radius, dr, lo, hi, beam), rr.columns(radius, dr, lo, hi, beam)
    print("radius", radius, "dr", dr, "box", lo, hi, "columns", len(want["w"]), "faces", int(want["face"].sum()),
          "sum w", rr.face_sum(want["w"]), "differ", int(np.count_nonzero(got["w"] != want["w"])))
    assert np.array_equal(got["col"], want["col"])
    assert np.array_equal(got["kstar"], want["kstar"])
    assert np.array_equal(got["face"], want["face"])
    assert np.array_equal(got["w"], want["w"])                     # bit for bit (no NaN: +0.0 without a face)
    assert np.array_equal(got["cell"][want["kstar"] >= 0], want["cell"][want["kstar"] >= 0])
    assert not np.signbit(got["w"]).any() and np.all(got["w"][~got["face"]] == 0.0) and np.all(got["w"][got["face"]] > 0.0)
    return want


def box(half):
    return [-half] * 3, [half] * 3


@pytest.mark.parametrize("cells", ["cubic", "box", "physical"])
def test_rule_on_every_column(rh, cells):
    """Every radius of the list in a +-10 box that contains the sphere; `physical`: cell sizes as the test grids have them."""
    dr = {"cubic": CUBIC, "box": BOX, "physical": tuple(k * D for k in BOX)}[cells]
    lo, hi = box(12 if cells != "cubic" else 10)
    for cells_r in RADII:
        radius = cells_r * dr[0]
        ref = check(rh, radius, dr, lo, hi)
        faces = int(ref["face"].sum())
        if cells_r < min(dr) / dr[0]:                               # the own cell only: six faces of weight 1/6
            assert faces == 6 and np.all(ref["w"][ref["face"]] == 1.0 / 6.0) and np.all(ref["kstar"][ref["face"]] == 0)
            assert sorted(ref["col"][ref["face"]][:, 0]) == [0, 1, 2, 3, 4, 5]
        else:
            assert faces > 6
        # every within-cell column pair: the two sheets of an axis have the same number of faces on a symmetric box
        for axis in range(3):
            assert int(ref["face"][ref["col"][:, 0] == 2 * axis].sum()) == int(ref["face"][ref["col"][:, 0] == 2 * axis + 1].sum())


def test_cells_exactly_on_the_sphere(rh):
    """Cubic cells of size 1, radius 3: (1, 2, 2) and (0, 0, 3) lie exactly on the sphere and are within, so the columns
    through them have k* there."""
    lo, hi = box(10)
    ref = check(rh, 3.0, CUBIC, lo, hi)
    at = {tuple(c): (int(k), bool(f)) for c, k, f in zip(ref["col"], ref["kstar"], ref["face"])}
    assert at[(5, 0, 0)] == (3, True) and at[(4, 0, 0)] == (3, True)            # +z and -z sheets, oa = ob = 0
    assert at[(5, 1, 2)] == (2, True) and at[(1, 2, 2)] == (1, True) and at[(3, 1, 2)] == (2, True)
    assert at[(5, 2, 2)] == (1, True) and at[(5, 3, 0)] == (0, True) and at[(5, 3, 1)] == (-1, False)


def test_asymmetric_box_smaller_than_the_sphere(rh):
    """lo != -hi, and the box ends two cells from the source on one side of x and three on one side of z while the radius is
    5.3 cells: a column that ends on the box's surface has no face (the kept loss has its term), the others keep theirs."""
    lo, hi = [-2, -9, -8], [9, 7, 3]
    for dr in (CUBIC, BOX):
        radius = 5.3 * dr[0]
        cut, free = check(rh, radius, dr, lo, hi), rr.columns(radius, dr, [-12] * 3, [12] * 3)
        surface = np.array([any(c[e] in (lo[e], hi[e]) for e in range(3)) for c in cut["cell"]])
        assert not cut["face"][surface & (cut["kstar"] >= 0)].any() and (surface & (cut["kstar"] >= 0)).any()
        # a face of the cut box is a face of the free sphere with the same k* and w, and there are fewer of them
        free_at = {tuple(c): (int(k), float(w)) for c, k, f, w in zip(free["col"], free["kstar"], free["face"], free["w"]) if f}
        n = 0
        for c, k, f, w in zip(cut["col"], cut["kstar"], cut["face"], cut["w"]):
            if f:
                assert free_at[tuple(c)] == (int(k), float(w))
                n += 1
        assert 0 < n < len(free_at)
        assert rr.face_sum(cut["w"]) < rr.face_sum(free["w"])
    check(rh, 1e200, CUBIC, lo, hi)                                  # R2 = +inf: every column ends on the surface, no face
    assert not rr.columns(1e200, CUBIC, lo, hi)["face"].any()


def test_cone_beam(rh):
    """A cone: a column whose cell is beam-unlit has no face; the lit faces are the unbeamed ones, same k* and w."""
    lo, hi = box(10)
    for dr in (CUBIC, BOX):
        radius = 6.2 * dr[0]
        cone, bare = check(rh, radius, dr, lo, hi, CONE), rr.columns(radius, dr, lo, hi)
        lit = np.array([bool(br.lit_offsets(CONE, dr, *c)) for c in bare["cell"]])
        assert np.array_equal(cone["face"], bare["face"] & lit) and np.array_equal(cone["kstar"], bare["kstar"])
        assert np.array_equal(cone["w"], np.where(lit, bare["w"], 0.0))
        assert 0 < cone["face"].sum() < bare["face"].sum()
    check(rh, 4.0, CUBIC, lo, hi, (br.BICONE, (0.0, 1.0, 0.0), 0.5))


def test_tiling_identity(rh):
    """The exposed faces of the staircase tile the sphere: |sum of w - 1| <= 1e-3 for radius >= 5 max(dr) in a box that
    contains the sphere (the header's weights, added in the fixed order)."""
    worst = 0.0
    for dr in (CUBIC, BOX):
        for cells_r in (5.0, 5.3, 7.7, 10.0, 16.0):
            radius = cells_r * max(dr)
            hi = [int(radius / x) + 2 for x in dr]
            lo = [-h for h in hi]
            assert all(radius < (h - 1) * x for h, x in zip(hi, dr))
            got = header_columns(rh, radius, dr, lo, hi)
            sw, ref = rr.face_sum(got["w"]), rr.face_sum(rr.columns(radius, dr, lo, hi)["w"])
            print("dr", dr, "radius", cells_r, "max(dr): sum of w", repr(sw), "- 1 =", sw - 1.0)
            assert sw == ref
            assert abs(sw - 1.0) <= 1e-3
            worst = max(worst, abs(sw - 1.0))
    print("worst", worst)


def test_face_sum_restated(rh):
    rng = np.random.default_rng(20261019)
    for n in (0, 1, 6, 63, 64, 255, 256, 257, 1536, 3456, 70000):
        v = rng.random(n) * 10.0 ** rng.integers(-30, 30, n)
        got = rh.rh_face_sum(v.ctypes.data_as(C.POINTER(C.c_double)), n)
        want = rr.face_sum(v)
        print(n, got, want)
        assert got == want
    six = np.full(6, 3.0e50 * (1.0 / 6.0))
    assert rr.face_sum(six) == rh.rh_face_sum(six.ctypes.data_as(C.POINTER(C.c_double)), 6)


def test_reference_on_the_oracle(pkg, orc, otables):
    """The pieces the GPU test composes, on the CPU: the restated predicate is horizon_reference's on a cube; the expected
    terms of the periodic 16^3 case are positive exactly on the faces; at zero columns every rim cell's photo_out is the
    oracle's po0, so the reference's loss / po0 is its sum of w."""
    import horizon_reference as hr
    r = range(-6, 7)
    for dr in (CUBIC, BOX):
        for radius in (0.0, 3.0, 5.3):
            for o in ((i, j, k) for i in r for j in r for k in r):
                assert rr.within(radius, dr, o) == bool(hr.within_offsets(radius, dr, *o)), (radius, dr, o)
    case = br.periodic_case(pkg, 16, "mixed", [(5, 6, 4), (12, 9, 11)], [3.0e7, 8.0e6])
    radius = 5.3 * float(case.dr[0])
    lo, hi = rr.final_box(case, 0, 1)
    assert (lo, hi) == ([-8] * 3, [7] * 3)
    terms, rule = rr.source_terms(pkg, orc, otables, case, "host_rim16", 0, radius, lo, hi)
    assert terms.size == 6 * 256 and np.array_equal(terms > 0, rule["face"]) and not np.signbit(terms).any()
    own = rr.cell_photo_out(pkg, orc, otables, case, "host_rim16", 0, (0, 0, 0))
    po0 = float(orc.photoion_rates(otables, [0.0] * 6, float(case.vol), float(case.flux[0]), 1.0, True)[20])
    print("faces", int(rule["face"].sum()), "loss", rr.face_sum(terms), "own cell's photo_out", own, "at zero columns", po0)
    assert 0 < rr.face_sum(terms) < own < po0
    assert abs(rr.face_sum(po0 * rule["w"]) / po0 - rr.face_sum(rule["w"])) <= 1e-12


def test_bindings_have_the_four_calls(pkg):
    names = ("c2r_enable_horizon_loss", "c2r_get_horizon_loss_enabled", "c2r_get_horizon_loss", "c2r_download_horizon_rim")
    assert all(hasattr(pkg.HipEngine, m) for m in ("enable_horizon_loss", "horizon_loss", "horizon_rim"))
    f = (ROOT / "c2-ray3dm1d_helium_amd" / "fortran" / "c2ray_hip_binding.f90").read_text()
    h = (ROOT / "include" / "c2ray_hip.h").read_text()
    for name in names:
        assert name in pkg._lib.SYMBOLS, name
        assert f'bind(C, name="{name}")' in f, name
    assert "int c2r_enable_horizon_loss(c2r_ctx *ctx, int on);" in h
    assert "int c2r_get_horizon_loss_enabled(const c2r_ctx *ctx);" in h
    assert "int c2r_get_horizon_loss(c2r_ctx *ctx, int nsrc, double *per_source, double *total);" in h
    assert "int c2r_download_horizon_rim(c2r_ctx *ctx, int *ns, int extent[3], double *terms, long long capacity);" in h
    text = h + (ROOT / "c2-ray3dm1d_helium_amd" / "csrc" / "c2ray_horizon.hpp").read_text()
    assert "THERE IS NO HORIZON LOSS unless c2r_enable_horizon_loss" in text and "no longer closes the photon budget" not in text
