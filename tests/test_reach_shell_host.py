"""The reach-cut shell order of open boundaries (csrc/c2ray_shell.hpp: reach_shell, reach_decode, reach_position,
reach_short_characteristic) on the CPU, through a small harness of its own (tests/reach_shell_harness.cpp).

A source reaches l_d <= 0 <= r_d cells per axis; shell s of it is the L-infinity shell cut at that box and occupies the
positions [E(s-1), E(s)) of a column array, E(s) = prod_d (min(r_d, s) - max(l_d, -s) + 1).
"""
import ctypes as C
import itertools
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def rs():
    so = ROOT / "tests" / "_reach_shell_harness.so"
    src = ROOT / "tests" / "reach_shell_harness.cpp"
    hdrs = list((ROOT / "c2-ray3dm1d_helium_amd" / "csrc").glob("*.hpp"))
    if not so.exists() or so.stat().st_mtime < max(p.stat().st_mtime for p in [src] + hdrs):
        subprocess.run(["g++", "-O2", "-ffp-contract=off", "-mfma", "-fPIC", "-shared", "-std=c++17", "-o", str(so), str(src)],
                       check=True)
    lib = C.CDLL(str(so))
    for name in ("rs_cells", "rs_shell_cells", "rs_position"):
        getattr(lib, name).restype = C.c_longlong
    return lib


def box(l, r):
    return (C.c_int * 3)(*l), (C.c_int * 3)(*r)


def small_boxes():
    """Every reach with |l_d|, r_d <= 4: 15 625 boxes."""
    for l in itertools.product(range(-4, 1), repeat=3):
        for r in itertools.product(range(0, 5), repeat=3):
            yield l, r


def random_boxes(n, top, seed):
    rng = np.random.default_rng(seed)
    for _ in range(n):
        yield tuple(int(-x) for x in rng.integers(0, top + 1, 3)), tuple(int(x) for x in rng.integers(0, top + 1, 3))


def test_entries_of_a_block():
    """E(s) written out here, against which the harness's reach_cells is checked below."""
    l, r = (0, -3, -1), (5, 2, 0)
    e = lambda s: int(np.prod([min(b, s) - max(a, -s) + 1 for a, b in zip(l, r)])) if s >= 0 else 0
    assert [e(s) for s in range(-1, 7)] == [0, 1, 2 * 3 * 2, 3 * 5 * 2, 4 * 6 * 2, 5 * 6 * 2, 6 * 6 * 2, 6 * 6 * 2]


def test_cells_and_shell_counts(rs):
    for l, r in list(random_boxes(50, 12, 7)) + [((0, 0, 0), (23, 23, 23)), ((-6, -12, -11), (17, 11, 12))]:
        cl, cr = box(l, r)
        smax = max(max(-a for a in l), max(r))
        for s in range(-1, smax + 3):
            e = int(np.prod([min(b, s) - max(a, -s) + 1 for a, b in zip(l, r)])) if s >= 0 else 0
            assert rs.rs_cells(cl, cr, s) == e, (l, r, s)
            if s >= 0:
                e1 = int(np.prod([min(b, s - 1) - max(a, -s + 1) + 1 for a, b in zip(l, r)])) if s >= 1 else 0
                assert rs.rs_shell_cells(cl, cr, s) == e - e1, (l, r, s)
        assert rs.rs_cells(cl, cr, smax) == int(np.prod([b - a + 1 for a, b in zip(l, r)]))


def test_thread_map_is_a_bijection_on_every_small_box(rs):
    """decode o position is the identity, positions fill [0, E(smax)) exactly once, shell s lies in [E(s-1), E(s)): every
    reach with |l_d|, r_d <= 4."""
    n = 0
    for l, r in small_boxes():
        assert rs.rs_check_box(*box(l, r)) == 0, (l, r)
        n += 1
    assert n == 15625


def test_thread_map_on_random_boxes(rs):
    """... and three hundred random reaches up to 12."""
    for l, r in random_boxes(300, 12, 20261):
        assert rs.rs_check_box(*box(l, r)) == 0, (l, r)


@pytest.mark.parametrize("cap", range(0, 7))
def test_uncut_reach_is_the_shell_order(rs, cap):
    """l = -cap, r = cap: shell_decode and shell_position entry for entry."""
    assert rs.rs_check_uncut(cap) == 0


def test_position_of_a_corner_source(rs):
    """A source in the corner (1,1,1) of a 4^3 mesh, written out: shell s holds (s+1)^3 - s^3 cells -- the +k face of
    (s+1)^2, the +j face of (s+1) s, the +i face of s^2."""
    l, r = box((0, 0, 0), (3, 3, 3))
    assert [rs.rs_shell_cells(l, r, s) for s in range(4)] == [1, 7, 19, 37]
    assert rs.rs_position(l, r, 0, 0, 0) == 0
    assert rs.rs_position(l, r, 0, 0, 1) == 1 and rs.rs_position(l, r, 1, 1, 1) == 4    # +k face of shell 1
    assert rs.rs_position(l, r, 0, 1, 0) == 5 and rs.rs_position(l, r, 1, 1, 0) == 6    # +j face
    assert rs.rs_position(l, r, 1, 0, 0) == 7                                            # +i face
    assert rs.rs_position(l, r, 0, 0, 2) == 8 and rs.rs_position(l, r, 3, 3, 3) == 27 + 15
    assert rs.rs_position(l, r, 3, 2, 2) == 63


def test_fast_corners_equal_the_general_ones(rs):
    """Shells >= 2: the four corner positions of the fast sweep equal the general position of the same corner cells
    wherever the weight is non-zero, every corner position is below E(s-1), weights and path are the uncut fast path's
    bits.  Every reach with |l_d|, r_d <= 4 and three hundred random ones up to 12."""
    cells = 0
    n = C.c_longlong(0)
    for l, r in itertools.chain(small_boxes(), random_boxes(300, 12, 4711)):
        assert rs.rs_check_corners(*box(l, r), C.byref(n)) == 0, (l, r)
        cells += n.value
    assert cells > 1_000_000


def test_host_sweep_in_the_cut_order_equals_the_mesh_ordered_one(rs):
    """The HI column of every cell of an open box, swept on the host with the product's functions in the cut shell order
    (shells >= 2 through the fast corners, zero-weight corners from the nearest cell that exists) and in mesh order with
    the general short_characteristic: the same bits in every cell.  A corner, an edge, a face, an interior source and
    lopsided boxes."""
    rs.rs_check_sweep.restype = C.c_longlong
    rng = np.random.default_rng(99)
    boxes = [((0, 0, 0), (11, 11, 11)), ((-11, -11, -11), (0, 0, 0)), ((-5, 0, -11), (6, 11, 0)), ((-4, -10, 0), (8, 0, 12)),
             ((-6, -7, -5), (5, 4, 6)), ((0, -3, -1), (12, 5, 4)), ((0, 0, 0), (0, 9, 3)), ((-2, 0, 0), (2, 0, 0))]
    for l, r in boxes + list(random_boxes(40, 9, 31)):
        ncell = int(np.prod([b - a + 1 for a, b in zip(l, r)]))
        u = np.ascontiguousarray(1.0e17 * np.exp(rng.normal(0.0, 1.5, ncell)))
        assert rs.rs_check_sweep(*box(l, r), u.ctypes.data_as(C.POINTER(C.c_double))) == 0, (l, r)
