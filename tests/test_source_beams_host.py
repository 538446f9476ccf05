"""Beamed point sources (c2r_set_source_beams) on the CPU.

1. The predicate of csrc/c2ray_beam.hpp -- the code the kernels run per lane -- compiled for the host (tests/beam_harness.cpp)
   against the NumPy restatement of tests/beam_reference.py over every offset of a 9 x 9 x 9 cube around the source, on cubic
   cells and on cells with dr = (d, 1.25 d, 0.75 d), for beams that include the exact-edge cases.
2. The reference itself against the oracle: without beams the fold is the oracle's own pass; the wall case has the columns
   and the rounds tests/test_gpu_source_beams.py relies on.
3. The notes of the gfx950 code object: no k_rates_beam instantiation has a private segment, the isothermal one-SED ones fit
   the waves their __launch_bounds__ asks for, and every k_rates instantiation has the figures recorded for the parent commit
   (profiles/source_beams_resources.json).

A note on the 45-degree cone.  No double squares to exactly 0.5 (0.7071067811865475^2 rounds to 0.4999999999999999, its upper
neighbour's to 0.5000000000000001), so for axis (0,0,1) the cells with di^2 + dj^2 == dk^2 are never exactly on a cone a caller
can set: with the lower neighbour they are lit, with sqrt(0.5) itself they are not, and both are checked.  The case whose edge
IS exact is axis (1,1,0) with cos_half = 0.5: K = 0.25 * 2 = 0.5, and on cubic cells every cell with
2 (di + dj)^2 == di^2 + dj^2 + dk^2, such as (1,0,1), lies on the cone with dot*dot == K*d2 bit for bit: lit.
"""
import ctypes as C
import json
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import beam_reference as br
from code_object import READELF, kernel_notes

ROOT = Path(__file__).resolve().parent.parent
HALF = 4
D = 2.3e24                                   # a cell size of the order the test grids have, cm; no power of two
CELLS = {"cubic": (D, D, D), "box": (D, 1.25 * D, 0.75 * D)}
C45_LIT, C45_DARK = 0.7071067811865475, 0.7071067811865476      # the two doubles around sqrt(1/2)
BEAMS = [
    (br.CONE, (0.0, 0.0, 1.0), C45_LIT),
    (br.CONE, (0.0, 0.0, 1.0), C45_DARK),
    (br.CONE, (1.0, 1.0, 0.0), 0.5),         # the exact edge
    (br.BICONE, (1.0, 1.0, 0.0), 0.5),
    (br.CONE, (0.0, 0.0, 1.0), 0.0),         # a half space, its boundary plane included
    (br.BICONE, (0.0, 0.0, 1.0), 0.0),       # everything
    (br.CONE, (0.0, 0.0, 1.0), 1.0),         # the ray along +z alone
    (br.BICONE, (0.0, -3.0, 0.0), 1.0),      # the line along y, axis not normalised and pointing down
    (br.CONE, (1.0, 2.0, -1.0), float(np.cos(np.radians(30.0)))),
    (br.BICONE, (-2.0, 0.5, 3.0), float(np.cos(np.radians(50.0)))),
    (br.CONE, (1.0e-3, 2.0e-3, 0.0), 0.9),
    (br.CONE, (7.0e5, 0.0, -7.0e5), 0.3),
]


@pytest.fixture(scope="module")
def bh():
    so = ROOT / "tests" / "_beam_harness.so"
    src = ROOT / "tests" / "beam_harness.cpp"
    hdrs = list((ROOT / "c2-ray3dm1d_helium_amd" / "csrc").glob("*.hpp"))
    if not so.exists() or so.stat().st_mtime < max(p.stat().st_mtime for p in [src] + hdrs):
        r = subprocess.run(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-std=c++17", "-o", str(so), str(src)],
                           capture_output=True, text=True)
        if r.returncode != 0:
            pytest.fail("tests/beam_harness.cpp does not compile against csrc/c2ray_beam.hpp:\n" + r.stderr[-2000:])
    lib = C.CDLL(str(so))
    lib.bh_beam_K.restype = C.c_double
    lib.bh_beam_K.argtypes = [C.c_double, C.POINTER(C.c_double)]
    lib.bh_lit_cube.restype = None
    lib.bh_lit_cube.argtypes = [C.c_int, C.POINTER(C.c_double), C.c_double, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_ubyte)]
    return lib


def cube_offsets():
    r = np.arange(-HALF, HALF + 1)
    dk, dj, di = np.meshgrid(r, r, r, indexing="ij")
    return di, dj, dk


def header_cube(bh, beam, dr):
    kind, axis, cos_half = beam
    w = 2 * HALF + 1
    out = (C.c_ubyte * (w * w * w))()
    bh.bh_lit_cube(int(kind), (C.c_double * 3)(*axis), float(cos_half), (C.c_double * 3)(*dr), HALF, out)
    return np.frombuffer(out, dtype=np.uint8).reshape(w, w, w).astype(bool)


@pytest.mark.parametrize("cells", sorted(CELLS))
def test_predicate_matches_the_header_on_every_offset_of_the_cube(bh, cells):
    dr = CELLS[cells]
    di, dj, dk = cube_offsets()
    for beam in BEAMS:
        assert bh.bh_beam_K(beam[2], (C.c_double * 3)(*beam[1])) == float(br.beam_K(beam[2], beam[1])), beam
        got, want = header_cube(bh, beam, dr), br.lit_offsets(beam, dr, di, dj, dk)
        print(cells, beam, "lit", int(got.sum()), "of", got.size, "differ", int(np.count_nonzero(got != want)))
        assert np.array_equal(got, want), beam
        assert got[HALF, HALF, HALF], "the source's own cell is lit"


def test_cells_exactly_on_the_cone_are_lit(bh):
    """Cubic cells.  Integer arithmetic says which cells lie exactly on the cone; the header must light every one of them."""
    dr = CELLS["cubic"]
    di, dj, dk = cube_offsets()
    r2 = di * di + dj * dj + dk * dk
    # axis (1,1,0), cos_half 1/2: cos^2 = (di + dj)^2 / (2 r^2) == 1/4
    edge = 2 * (di + dj) ** 2 == r2
    cone, bicone = header_cube(bh, BEAMS[2], dr), header_cube(bh, BEAMS[3], dr)
    assert edge.sum() > 20 and edge[HALF + 1, HALF, HALF + 1]                       # (di, dj, dk) = (1, 0, 1)
    assert np.all(bicone[edge]) and np.all(cone[edge & (di + dj >= 0)]) and not np.any(cone[edge & (di + dj < 0)])
    assert np.array_equal(bicone, 2 * (di + dj) ** 2 >= r2)                       # and nothing beyond the cone
    assert np.array_equal(cone, (2 * (di + dj) ** 2 >= r2) & (di + dj >= 0))
    # axis (0,0,1) at 45 degrees: cells with di^2 + dj^2 == dk^2, dk > 0 -- lit below sqrt(1/2), dark at sqrt(1/2) itself
    edge45 = (di * di + dj * dj == dk * dk) & (dk > 0)
    lit, dark = header_cube(bh, BEAMS[0], dr), header_cube(bh, BEAMS[1], dr)
    assert edge45.sum() > 10 and np.all(lit[edge45]) and not np.any(dark[edge45])
    assert np.array_equal(lit, (2 * dk * dk >= r2) & (dk >= 0)) and np.array_equal(lit & ~dark, edge45)
    # cos_half = 0: the half space with its boundary plane, and everything; cos_half = 1: the ray and the line
    assert np.array_equal(header_cube(bh, BEAMS[4], dr), dk >= 0) and np.all(header_cube(bh, BEAMS[5], dr))
    assert np.array_equal(header_cube(bh, BEAMS[6], dr), (di == 0) & (dj == 0) & (dk >= 0))
    assert np.array_equal(header_cube(bh, BEAMS[7], dr), (di == 0) & (dk == 0))


def test_binding_record_has_the_header_layout(pkg):
    b = pkg._lib.SourceBeam
    assert C.sizeof(b) == 40 and b.kind.offset == 0 and b.axis.offset == 8 and b.cos_half.offset == 32
    f = (ROOT / "c2-ray3dm1d_helium_amd" / "fortran" / "c2ray_hip_binding.f90").read_text()
    assert "type, bind(C) :: c2r_source_beam" in f
    assert hasattr(pkg.HipEngine, "set_source_beams") and hasattr(pkg.HipEngine, "source_beam")


# -- the reference against the oracle ----------------------------------------------------------------------------------------
def two_source_case(pkg, heat=False, seds=False):
    """Periodic 16^3 (reach 8 < subboxsize: one geometric round), mixed gas, two sources."""
    kw = dict(pl=np.array([1e6, 2e6]), qpl=np.array([5e5, 1e6])) if seds else {}
    return br.periodic_case(pkg, 16, "mixed", [(5, 6, 4), (12, 9, 11)], [3.0e7, 8.0e6], heat=heat, **kw)


def test_without_beams_the_fold_is_the_oracle_pass(pkg, orc, otables):
    case = two_source_case(pkg, heat=True)
    ref = br.compose(pkg, orc, otables, case, "host16_heat", [None, None])
    whole = case.oracle_pass(pkg, orc, otables)
    for k in br.GRIDS:
        assert np.array_equal(ref[k], whole[k]), k
    assert ref["nbox"] == [1, 1] and whole["sum_nbox"] == 2
    beamed = br.compose(pkg, orc, otables, case, "host16_heat", [(br.CONE, (0.0, 0.0, 1.0), C45_LIT), None])
    lit = br.lit_cells(case, 0, (br.CONE, (0.0, 0.0, 1.0), C45_LIT))
    alone2 = br.source_alone(pkg, orc, otables, case, "host16_heat", 2)[0]
    assert 0 < lit.sum() < lit.size // 2
    for k in br.GRIDS:       # where source 1 is dark the grid is source 2's alone; where it is lit, the whole pass's
        m = np.tile(lit, ref[k].size // lit.size)
        assert np.array_equal(beamed[k][~m], (0.0 + alone2[k])[~m]) and np.array_equal(beamed[k][m], whole[k][m]), k


@pytest.mark.parametrize("heat", [False, True])
def test_wall_case_has_the_columns_and_rounds_the_gpu_test_relies_on(pkg, orc, otables, heat):
    """Unbeamed the oracle needs both rounds; every lit cell on the surface of the first sub-box lies on its +x face and has
    an incoming HI column >= max_coldensh, so the beamed source loses exactly 0.0 through it and stops after one round."""
    case = br.wall_case(pkg, heat=heat)
    key = "wall_heat" if heat else "wall"
    _, nbox, loss, _ = br.source_alone(pkg, orc, otables, case, key, 1)
    cols = br.wall_incoming_columns(pkg, orc, otables, case, key)
    print("oracle rounds", nbox, "loss", loss, "lit surface cells", len(cols), "smallest N_in(HI)", min(c for _, c in cols))
    assert nbox == 2 and loss > 0
    assert len(cols) > 50 and all(o[0] == br.ab.SUBBOXSIZE for o, _ in cols)
    assert all(c >= br.fl.MAX_COLDENSH for _, c in cols)


# -- the code object ---------------------------------------------------------------------------------------------------------
def test_rates_kernels_in_the_code_object(pkg):
    """k_rates_beam: eight instantiations, none with a private segment; the isothermal one-SED ones within the vector registers
    of the waves per SIMD their __launch_bounds__ asks for (512 registers per lane and SIMD, allocated in eights).  k_rates: the
    eight instantiations, each with the figures the parent commit's library has (profiles/source_beams_resources.json, 'before'),
    and the file's 'after' is what the library holds."""
    if not Path(READELF).exists():
        pytest.skip("llvm-readelf not present")
    notes = kernel_notes(pkg.build())
    beam = {n: v for n, v in notes.items() if "12k_rates_beamILb" in n}
    plain = {n: v for n, v in notes.items() if "7k_ratesILb" in n}
    assert len(beam) == 8 and len(plain) == 8, sorted(notes)
    for n, v in sorted({**plain, **beam}.items()):
        print(n[:48], v)
    assert {n: v for n, v in beam.items() if v["private_segment"]} == {}
    src = (ROOT / "c2-ray3dm1d_helium_amd" / "csrc" / "c2ray_hip.hip").read_text()
    waves = int(re.search(r"#define C2R_RATES_WAVES_ISO (\d+)", src).group(1))
    iso = {n: v for n, v in beam.items() if re.search(r"12k_rates_beamILb0ELb0ELb[01]E", n)}
    assert len(iso) == 2
    for n, v in iso.items():
        alloc = -(-(-(-v["vgpr"] // 4) * 4 + v["agpr"]) // 8) * 8
        assert alloc <= 512 // waves, (n, v, alloc, waves)
    rec = json.loads((ROOT / "profiles" / "source_beams_resources.json").read_text())
    keys = ("vgpr", "agpr", "sgpr", "private_segment", "lds")
    before = {v["mangled"]: {k: v[k] for k in keys} for v in rec["before"].values()}
    after = {v["mangled"]: {k: v[k] for k in keys} for v in rec["after"].values()}
    assert before == plain
    assert after == {**plain, **beam}
