"""Photon horizons (c2r_set_source_horizons) on the CPU.

1. The predicates of csrc/c2ray_horizon.hpp -- the code the kernels run per lane -- compiled for the host
   (tests/horizon_harness.cpp) against the NumPy restatement of tests/horizon_reference.py, with == on every offset of a
   25 x 25 x 25 cube around the source (|o| <= 12):
     * cubic cells whose dr is a power of two, radius 5 dr and 3 dr: every product is exact, so integer arithmetic says which
       cells are within, the Pythagorean ones on the sphere included;
     * cells with dr = (d, 1.25 d, 0.75 d): a radius between two neighbouring values of d2, and one whose square IS a cell's d2;
     * radius 0 (the own cell only) and 1e200 (R2 overflows to +inf: everything);
     * a cone with a horizon through cut_lit against the product of the two NumPy predicates.
2. The reference against the oracle at 16^3: all horizons inf is beam_reference.compose, radius 0 leaves the own cell only.
3. The bindings, and the notes of the gfx950 code object against profiles/source_horizon_resources.json.
"""
import ctypes as C
import itertools
import json
import subprocess
from pathlib import Path

import numpy as np
import pytest

import beam_reference as br
import horizon_reference as hr
import mix_reference as mr
from code_object import READELF, kernel_notes
from test_source_beams_host import two_source_case

ROOT = Path(__file__).resolve().parent.parent
HALF = 12
P2 = 2.0 ** 81                               # 2.4e24 cm: a cell size of the order the test grids have, a power of two
D = 2.3e24                                   # and one that is none
BOX = tuple(k * D for k in mr.DR_FACTORS)
INF = float("inf")


@pytest.fixture(scope="module")
def hh():
    so = ROOT / "tests" / "_horizon_harness.so"
    src = ROOT / "tests" / "horizon_harness.cpp"
    hdrs = list((ROOT / "c2-ray3dm1d_helium_amd" / "csrc").glob("*.hpp"))
    if not so.exists() or so.stat().st_mtime < max(p.stat().st_mtime for p in [src] + hdrs):
        r = subprocess.run(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-std=c++17", "-o", str(so), str(src)],
                           capture_output=True, text=True)
        if r.returncode != 0:
            pytest.fail("tests/horizon_harness.cpp does not compile against csrc/c2ray_horizon.hpp:\n" + r.stderr[-2000:])
    lib = C.CDLL(str(so))
    d3 = C.POINTER(C.c_double)
    lib.hh_horizon_R2.restype = C.c_double
    lib.hh_horizon_R2.argtypes = [C.c_double]
    lib.hh_within_cube.restype = None
    lib.hh_within_cube.argtypes = [C.c_double, d3, C.c_int, C.POINTER(C.c_ubyte)]
    lib.hh_cut_cube.restype = None
    lib.hh_cut_cube.argtypes = [C.c_int, d3, C.c_double, C.c_double, d3, C.c_int, C.POINTER(C.c_ubyte)]
    return lib


def cube_offsets():
    r = np.arange(-HALF, HALF + 1)
    dk, dj, di = np.meshgrid(r, r, r, indexing="ij")
    return di, dj, dk


def at(cube, o):
    return bool(cube[o[2] + HALF, o[1] + HALF, o[0] + HALF])


def header_within(hh, radius, dr):
    w = 2 * HALF + 1
    out = (C.c_ubyte * (w * w * w))()
    hh.hh_within_cube(float(radius), (C.c_double * 3)(*dr), HALF, out)
    return np.frombuffer(out, dtype=np.uint8).reshape(w, w, w).astype(bool)


def header_cut(hh, beam, radius, dr):
    kind, axis, cos_half = (0, (0.0, 0.0, 0.0), 0.0) if beam is None else beam
    w = 2 * HALF + 1
    out = (C.c_ubyte * (w * w * w))()
    hh.hh_cut_cube(int(kind), (C.c_double * 3)(*axis), float(cos_half), float(radius), (C.c_double * 3)(*dr), HALF, out)
    return np.frombuffer(out, dtype=np.uint8).reshape(w, w, w).astype(bool)


def check(hh, radius, dr):
    """The header's two routes against the restatement, == on every cell; returns the cube."""
    di, dj, dk = cube_offsets()
    got, want = header_within(hh, radius, dr), hr.within_offsets(radius, dr, di, dj, dk)
    print("radius", radius, "dr", dr, "within", int(got.sum()), "of", got.size, "differ", int(np.count_nonzero(got != want)))
    assert hh.hh_horizon_R2(float(radius)) == float(hr.horizon_R2(radius))
    assert np.array_equal(got, want), radius
    assert np.array_equal(header_cut(hh, None, radius, dr), want), radius
    assert got[HALF, HALF, HALF], "the source's own cell is within"
    return got


def signed_permutations(o):
    return {tuple(s * x for s, x in zip(sg, p)) for p in itertools.permutations(o) for sg in itertools.product((1, -1), repeat=3)}


def test_cubic_power_of_two_cells_are_exact(hh):
    """dr = 2^81: every product and sum of the rule is exact, so within iff di^2 + dj^2 + dk^2 <= (radius/dr)^2 in integers."""
    dr = (P2, P2, P2)
    di, dj, dk = cube_offsets()
    r2 = di * di + dj * dj + dk * dk
    five, three = check(hh, 5 * P2, dr), check(hh, 3 * P2, dr)
    assert np.array_equal(five, r2 <= 25) and np.array_equal(three, r2 <= 9)
    for o in signed_permutations((3, 4, 0)) | signed_permutations((0, 0, 5)):      # exactly on the sphere of radius 5
        assert at(five, o), o
    for o in signed_permutations((3, 4, 1)):
        assert not at(five, o), o
    for o in signed_permutations((1, 2, 2)):                                         # exactly on the sphere of radius 3
        assert at(three, o), o
    for o in signed_permutations((2, 2, 2)):
        assert not at(three, o) and at(five, o), o


def test_cells_that_are_no_cubes(hh):
    """dr = (d, 1.25 d, 0.75 d): the lit set follows physical lengths, and a cell whose d2 is R2 bit for bit is within."""
    di, dj, dk = cube_offsets()
    xs, ys, zs = BOX[0] * di.astype(np.float64), BOX[1] * dj.astype(np.float64), BOX[2] * dk.astype(np.float64)
    d2 = (xs * xs + ys * ys) + zs * zs
    values = np.unique(d2)
    lo = int(np.searchsorted(values, (4.4 * D) ** 2))
    gaps = (values[lo + 1: lo + 40] - values[lo: lo + 39]) / values[lo: lo + 39]
    k = lo + int(np.argmax(gaps))                            # two neighbouring values of d2 far enough apart to aim between
    radius = float(np.sqrt(0.5 * (values[k] + values[k + 1])))
    assert values[k] < radius * radius < values[k + 1] and gaps.max() > 1e-3
    got = check(hh, radius, BOX)
    assert np.array_equal(got, d2 <= values[k]) and not np.array_equal(got, (di * di + dj * dj + dk * dk) <= (radius / D) ** 2)
    # radius = dr2 * 4: its square is the d2 of (0, +-4, 0) -- (0 + ys*ys) + 0 -- exactly
    radius = BOX[1] * 4.0
    assert radius * radius == d2[HALF, HALF + 4, HALF]
    got = check(hh, radius, BOX)
    assert at(got, (0, 4, 0)) and at(got, (0, -4, 0)) and not at(got, (0, 5, 0))
    assert at(got, (5, 0, 0)) and not at(got, (6, 0, 0)) and at(got, (0, 0, 6)) and not at(got, (0, 0, 7))   # 5 d, 6 * 0.75 d <= 5 d
    inner = float(np.nextafter(radius, 0.0))
    assert not at(check(hh, inner, BOX), (0, 4, 0))


def test_radius_zero_and_overflowing_radius(hh):
    for dr in ((P2, P2, P2), BOX):
        zero = check(hh, 0.0, dr)
        assert zero.sum() == 1 and zero[HALF, HALF, HALF]
        assert hr.horizon_R2(1e200) == INF
        assert np.all(check(hh, 1e200, dr))
        di, dj, dk = cube_offsets()
        assert np.all(header_cut(hh, None, INF, dr)) and np.all(hr.within_offsets(INF, dr, di, dj, dk))
        assert np.all(hr.within_offsets(None, dr, di, dj, dk))


@pytest.mark.parametrize("cells", ["cubic", "box"])
def test_cone_and_horizon_is_the_product_of_the_two_predicates(hh, cells):
    dr = (D, D, D) if cells == "cubic" else BOX
    di, dj, dk = cube_offsets()
    beams = [(br.CONE, (0.0, 0.0, 1.0), 0.7071067811865475), (br.BICONE, (1.0, 1.0, 0.0), 0.5),
             (br.CONE, (1.0, 2.0, -1.0), float(np.cos(np.radians(30.0))))]
    for beam in beams:
        for radius in (0.0, 4.5 * D, 7.0 * D, 1e200, INF):
            got = header_cut(hh, beam, radius, dr)
            want = br.lit_offsets(beam, dr, di, dj, dk) & hr.within_offsets(radius, dr, di, dj, dk)
            print(cells, beam, radius, "lit", int(got.sum()), "differ", int(np.count_nonzero(got != want)))
            assert np.array_equal(got, want) and np.array_equal(want, hr.lit_offsets(beam, radius, dr, di, dj, dk)), (beam, radius)
            assert got[HALF, HALF, HALF]
        both = header_cut(hh, beam, 4.5 * D, dr)
        assert 0 < both.sum() < header_cut(hh, beam, INF, dr).sum() and both.sum() < header_within(hh, 4.5 * D, dr).sum()


# -- the reference against the oracle ----------------------------------------------------------------------------------------
def test_composition_on_the_oracle(pkg, orc, otables):
    """Periodic 16^3, two sources: with every horizon inf the fold is beam_reference.compose's (the oracle's own pass, as
    tests/test_source_beams_host.py shows); with radius 0 exactly the source's own cell is non-zero."""
    case = two_source_case(pkg, heat=True)
    plain = br.compose(pkg, orc, otables, case, "host16_heat", [None, None])
    for horizons in ([INF, INF], [None, INF], [1e200, None]):
        ref = hr.compose(pkg, orc, otables, case, "host16_heat", horizons)
        for k in hr.GRIDS:
            assert np.array_equal(ref[k], plain[k]), (k, horizons)
        assert ref["nbox"] == [1, 1]
    ncell = 16 ** 3
    for ns in (1, 2):
        ref = hr.compose(pkg, orc, otables, case, "host16_heat", [0.0, 0.0], sources=[ns])
        i, j, k = (int(x) - 1 for x in case.srcpos[ns - 1])
        own = i + 16 * (j + 16 * k)
        for g in hr.GRIDS:
            nz = np.flatnonzero(ref[g])
            assert sorted(set(int(q) % ncell for q in nz)) == [own], (g, ns)
    dr = float(case.dr[0])
    part = hr.compose(pkg, orc, otables, case, "host16_heat", [4.5 * dr, None])
    w = hr.within_cells(case, 0, 4.5 * dr)
    alone2 = br.source_alone(pkg, orc, otables, case, "host16_heat", 2)[0]
    assert 0 < w.sum() < w.size // 4
    for g in hr.GRIDS:      # beyond the horizon of source 1 the grid is source 2's alone; within it, the whole pass's
        m = np.tile(w, part[g].size // w.size)
        assert np.array_equal(part[g][~m], (0.0 + alone2[g])[~m]) and np.array_equal(part[g][m], plain[g][m]), g


# -- the bindings and the code object ------------------------------------------------------------------------------------------
def test_bindings_have_the_two_calls(pkg):
    assert hasattr(pkg.HipEngine, "set_source_horizons") and hasattr(pkg.HipEngine, "get_source_horizon")
    assert "c2r_set_source_horizons" in pkg._lib.SYMBOLS and "c2r_get_source_horizon" in pkg._lib.SYMBOLS
    f = (ROOT / "c2-ray3dm1d_helium_amd" / "fortran" / "c2ray_hip_binding.f90").read_text()
    assert 'bind(C, name="c2r_set_source_horizons")' in f and 'bind(C, name="c2r_get_source_horizon")' in f
    h = (ROOT / "include" / "c2ray_hip.h").read_text()
    assert "int c2r_set_source_horizons(c2r_ctx *ctx, int nsrc, const double *radius);" in h
    assert "int c2r_get_source_horizon(const c2r_ctx *ctx, int ns, double *radius);" in h


def test_rates_kernels_in_the_code_object(pkg):
    """profiles/source_horizon_resources.json: every k_rates instantiation has the parent commit's figures ('before'), no
    k_rates_beam instantiation has a private segment or more than the 128 vector registers of the four waves per SIMD its
    __launch_bounds__ asks for, and 'after' is what the library holds."""
    if not Path(READELF).exists():
        pytest.skip("llvm-readelf not present")
    notes = kernel_notes(pkg.build())
    beam = {n: v for n, v in notes.items() if "12k_rates_beamILb" in n}
    plain = {n: v for n, v in notes.items() if "7k_ratesILb" in n}
    assert len(beam) == 8 and len(plain) == 8, sorted(notes)
    for n, v in sorted(beam.items()):
        print(n[:48], v)
        assert v["private_segment"] == 0 and v["vgpr"] + v["agpr"] <= 128, (n, v)
    rec = json.loads((ROOT / "profiles" / "source_horizon_resources.json").read_text())
    keys = ("vgpr", "agpr", "sgpr", "private_segment", "lds")
    before = {v["mangled"]: {k: v[k] for k in keys} for v in rec["before"].values()}
    after = {v["mangled"]: {k: v[k] for k in keys} for v in rec["after"].values()}
    assert {n: v for n, v in before.items() if "7k_ratesILb" in n} == plain
    assert after == {**plain, **beam}
