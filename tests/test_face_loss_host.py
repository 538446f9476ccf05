"""Escape maps (c2r_enable_face_loss) on the CPU.

1. The attribution rule, the face-cell index and the fixed-order sum of csrc/c2ray_face.hpp -- the code k_face_loss runs per
   lane -- compiled for the host (tests/face_harness.cpp) and run exhaustively: every mesh extent 1..6 per axis with unequal
   cell sizes, every open / periodic mask with an open axis, every source position, every cell of its reach.
2. The reference of tests/face_loss_reference.py against the oracle itself: where every box runs to its reach and all axes
   are open, the maps' total is the sum of the oracle-side terms over the region's surface.
"""
import ctypes as C
import math
import subprocess
from pathlib import Path

import numpy as np
import pytest

import face_loss_reference as fr
import open_boundary_cases as ob

ROOT = Path(__file__).resolve().parent.parent
DR = (1.0, 1.25, 0.75)      # |o| dr ties across axes exist (5 * 1.0 == 4 * 1.25, 3 * 1.0 == 4 * 0.75, 5 * 0.75 == 3 * 1.25)


@pytest.fixture(scope="module")
def fh():
    so = ROOT / "tests" / "_face_harness.so"
    src = ROOT / "tests" / "face_harness.cpp"
    hdrs = list((ROOT / "c2-ray3dm1d_helium_amd" / "csrc").glob("*.hpp"))
    if not so.exists() or so.stat().st_mtime < max(p.stat().st_mtime for p in [src] + hdrs):
        r = subprocess.run(["g++", "-O2", "-ffp-contract=off", "-mfma", "-fPIC", "-shared", "-std=c++17", "-o", str(so), str(src)],
                           capture_output=True, text=True)
        if r.returncode != 0:
            pytest.fail("tests/face_harness.cpp does not compile against csrc/c2ray_face.hpp:\n" + r.stderr[-2000:])
    lib = C.CDLL(str(so))
    lib.fh_face_sum.restype = C.c_double
    lib.fh_face_sum.argtypes = [C.POINTER(C.c_double), C.c_longlong]
    return lib


def test_every_cell_of_every_reach_gets_the_face_the_rule_gives(fh):
    """Every cell on an open mesh face gets exactly one face, one of its candidates, the one the tie rules name; a cell on no
    open face gets none; face-cell index, its inverse and the maps' offsets are a bijection onto the buffer."""
    counts, bad = (C.c_longlong * 4)(), (C.c_longlong * 6)()
    rc = fh.fh_sweep(6, (C.c_double * 3)(*DR), counts, bad)
    print("pairs", counts[0], "with a candidate", counts[1], "at edges and corners", counts[2], "decided by a tie rule", counts[3])
    names = ("no face or several", "face is no candidate", "face without candidate", "not the rule's face", "index is no bijection",
             "offset not reproduced")
    assert rc == 0 and not any(bad), dict(zip(names, bad))
    assert counts[1] > 0 and counts[2] > 0 and counts[3] > 0 and counts[0] > counts[1]


def _iv(*x):
    return (C.c_int * len(x))(*x)


def test_the_numpy_restatement_is_the_same_rule(fh):
    """tests/face_loss_reference.py's attribute / face_cell against the header's functions on random cells of random meshes."""
    rng = np.random.default_rng(7)
    dr = (C.c_double * 3)(*DR)
    hits = 0
    for _ in range(20000):
        n = [int(x) for x in rng.integers(1, 8, 3)]
        periodic = [bool(x) for x in rng.integers(0, 2, 3)]
        if all(periodic):
            continue
        m1 = [int(rng.integers(1, n[d] + 1)) if rng.random() < 0.5 else int(rng.choice([1, n[d]])) for d in range(3)]
        o = [int(rng.integers(-6, 7)) for _ in range(3)]
        want = fr.attribute(n, periodic, m1, o, DR)
        got = fh.fh_face_of_cell(_iv(*n), _iv(*[int(not p) for p in periodic]), _iv(*[x - 1 for x in m1]), _iv(*o), dr)
        assert got == (-1 if want is None else want), (n, periodic, m1, o)
        if want is not None:
            hits += 1
            assert fh.fh_face_cell_index(_iv(*n), want // 2, _iv(*[x - 1 for x in m1])) == fr.face_cell(n, want, m1)
    assert hits > 5000


def test_the_fixed_order_sum(fh):
    """face_sum: exact on numbers whose every partial sum is exact, and within the bound of a sum of n positive terms in
    another order (n * 2^-53 relative) of math.fsum on others; sizes around the block of 256 and its square."""
    rng = np.random.default_rng(3)
    dp = C.POINTER(C.c_double)
    for n in (0, 1, 63, 64, 255, 256, 257, 1000, 65536, 65537, 70001):
        ints = rng.integers(0, 1 << 20, n).astype(np.float64)
        assert fh.fh_face_sum(ints.ctypes.data_as(dp), n) == float(ints.sum())
        x = 10.0 ** rng.uniform(-3, 3, n)
        got, ref = fh.fh_face_sum(x.ctypes.data_as(dp), n), math.fsum(x)
        assert abs(got - ref) <= max(n, 1) * 2.0 ** -53 * ref
        assert fh.fh_face_sum(x.ctypes.data_as(dp), n) == got


def test_reference_total_is_the_surface_sum_of_the_oracle_terms(pkg, orc, otables):
    """case_several_rounds (N = 24, all axes open, every box runs to its reach): the total of the maps equals the sum over
    the region's surface of photo_out * vol / vol_ph from the oracle's columns, to 1e-13 relative (the project's bound for a
    loss summed in another order); every surface cell of every source carries a term and lands in exactly one map."""
    case = ob.case_several_rounds(pkg)
    n = case.n
    maps, per_source = fr.expected(pkg, orc, otables, case, "several_rounds")
    surface_cells = n ** 3 - (n - 2) ** 3
    terms_all = []
    for ns in range(len(case.flux)):
        terms = fr.cached_terms("several_rounds", ns)
        assert len(terms) == surface_cells and len({t[0] for t in terms}) == surface_cells
        assert all(t[2] > 0.0 for t in terms)
        assert sum(int(np.count_nonzero(a)) for a in per_source[ns].values()) == surface_cells
        terms_all += [t[2] for t in terms]
    want, got = math.fsum(terms_all), fr.total_of(maps)
    print("surface sum", want, "maps' total", got, "rel", abs(got - want) / want)
    assert want > 0 and abs(got - want) <= 1e-13 * want
    assert sorted(maps) == [0, 1, 2, 3, 4, 5] and all(maps[f].shape == (n, n) for f in maps)
