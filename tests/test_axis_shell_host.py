"""Boundaries per axis (c2r_set_boundaries_axes) on the CPU: the per-axis helpers of csrc/c2ray_shell.hpp -- the reach of an
axis, offset -> mesh index, cell -> offset -- and the reach-cut shell order on the mixed reaches they give, through a small
harness of its own (tests/axis_shell_harness.cpp).

Per axis of `mesh` cells, a source at the 1-based position pos, the reach cut at max_subbox (include/c2ray_hip.h):
  open:     l = -min(max_subbox, pos - 1),  r = min(max_subbox, mesh - pos)
  periodic: l = -min(max_subbox, mesh/2),   r = min(max_subbox, mesh/2 - 1 + mod(mesh, 2))
The cell at offset o lies at pos + o, modulo the mesh on a periodic axis and as it is on an open one.
"""
import ctypes as C
import itertools
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
FULL = 1150      # the reference's max_subbox: no cut on these meshes


@pytest.fixture(scope="module")
def ax():
    so = ROOT / "tests" / "_axis_shell_harness.so"
    src = ROOT / "tests" / "axis_shell_harness.cpp"
    hdrs = list((ROOT / "c2-ray3dm1d_helium_amd" / "csrc").glob("*.hpp"))
    if not so.exists() or so.stat().st_mtime < max(p.stat().st_mtime for p in [src] + hdrs):
        subprocess.run(["g++", "-O2", "-ffp-contract=off", "-mfma", "-fPIC", "-shared", "-std=c++17", "-o", str(so), str(src)],
                       check=True)
    return C.CDLL(str(so))


def expected_reach(mesh, pos, periodic, max_subbox):
    if periodic:
        return -min(max_subbox, mesh // 2), min(max_subbox, mesh // 2 - 1 + mesh % 2)
    return -min(max_subbox, pos - 1), min(max_subbox, mesh - pos)


def reach(ax, mesh, pos, periodic, max_subbox):
    l, r = C.c_int(99), C.c_int(-99)
    ax.ax_reach(mesh, pos, int(periodic), max_subbox, C.byref(l), C.byref(r))
    return l.value, r.value


AXES = [(mesh, pos, periodic) for mesh in range(1, 10) for pos in range(1, mesh + 1) for periodic in (False, True)]


@pytest.mark.parametrize("max_subbox", [FULL, 1, 2, 3])
def test_reach_is_the_formula(ax, max_subbox):
    for mesh, pos, periodic in AXES:
        l, r = reach(ax, mesh, pos, periodic, max_subbox)
        assert (l, r) == expected_reach(mesh, pos, periodic, max_subbox), (mesh, pos, periodic)
        assert l <= 0 <= r and r - l + 1 <= mesh
        if max_subbox == FULL and periodic:
            assert r - l + 1 == mesh        # a periodic axis is reached as a whole
        if max_subbox == FULL and not periodic:
            assert (pos + l, pos + r) == (1, mesh)


@pytest.mark.parametrize("max_subbox", [FULL, 1, 2, 3])
def test_offsets_and_mesh_indices_are_inverse_on_the_reach(ax, max_subbox):
    """Every axis length 1..9, every source position, both modes; with the reach as it is and shortened as by max_subbox =
    1..3.  Offset -> mesh index is a bijection between [l, r] and the cells reached and gives, on an open axis, pos + o
    itself; cell -> offset gives the offset back, lands in [l, r] for exactly the cells reached -- so a cell that a short
    reach leaves out is seen as outside, on an open axis as well, where its offset is the plain difference."""
    for mesh, pos, periodic in AXES:
        w = ax.ax_wrap_extent(mesh, int(periodic))
        assert w == (mesh if periodic else 0)
        l, r = reach(ax, mesh, pos, periodic, max_subbox)
        cells = [ax.ax_mesh_index(pos, o, w) for o in range(l, r + 1)]
        expect = [(pos - 1 + o) % mesh if periodic else pos - 1 + o for o in range(l, r + 1)]
        assert cells == expect, (mesh, pos, periodic)
        assert len(set(cells)) == len(cells) and all(0 <= c < mesh for c in cells)
        for o, c in zip(range(l, r + 1), cells):
            assert ax.ax_offset(c, pos, w) == o, (mesh, pos, periodic, o)
        for c in range(mesh):
            o = ax.ax_offset(c, pos, w)
            assert (l <= o <= r) == (c in cells), (mesh, pos, periodic, c, o)
            if not periodic:
                assert o == c + 1 - pos
            else:
                assert (pos - 1 + o) % mesh == c and -(mesh // 2) <= o <= mesh // 2 - 1 + mesh % 2


def test_short_reach_on_an_open_axis_written_out(ax):
    """The trap: mesh 9, source at 5, max_subbox 2 -- the reach [-2, 2] holds the cells 3..7.  Cell 1 lies at offset -4;
    taken modulo the width of the reach, or modulo the mesh relative to the reach's left end, it would land inside."""
    assert reach(ax, 9, 5, False, 2) == (-2, 2)
    assert [ax.ax_offset(c, 5, 0) for c in range(9)] == [-4, -3, -2, -1, 0, 1, 2, 3, 4]
    assert reach(ax, 9, 8, False, 2) == (-2, 1)
    assert [ax.ax_offset(c, 8, 0) for c in range(9)] == [-7, -6, -5, -4, -3, -2, -1, 0, 1]
    # the same source on a periodic axis: the cells 6, 7, 8 and, through the face, 0
    assert reach(ax, 9, 8, True, 2) == (-2, 2)
    assert [ax.ax_mesh_index(8, o, 9) for o in range(-2, 3)] == [5, 6, 7, 8, 0]
    assert [ax.ax_offset(c, 8, 9) for c in range(9)] == [2, 3, 4, -4, -3, -2, -1, 0, 1]


@pytest.mark.parametrize("periodic", list(itertools.product((0, 1), repeat=3)), ids=lambda p: "".join("po"[1 - v] for v in p))
@pytest.mark.parametrize("max_subbox", [FULL, 2])
def test_cut_shell_order_on_mixed_reaches(ax, periodic, max_subbox):
    """A (5,4,6) mesh, all eight masks, every source position: reach_position / reach_decode stay a bijection on the mixed
    reach, whose cells map one to one onto cells of the mesh and back; with the full reach a periodic axis is held as a
    whole, an open one from face to face, so every cell of the mesh is reached."""
    mesh = (5, 4, 6)
    cm, cp = (C.c_int * 3)(*mesh), (C.c_int * 3)(*periodic)
    reached = C.c_longlong(0)
    for src in itertools.product(*(range(1, n + 1) for n in mesh)):
        assert ax.ax_check_mixed_box(cm, (C.c_int * 3)(*src), cp, max_subbox, C.byref(reached)) == 0, src
        want = 1
        for n, p, per in zip(mesh, src, periodic):
            l, r = expected_reach(n, p, per, max_subbox)
            want *= r - l + 1
        assert reached.value == want
        if max_subbox == FULL:
            assert reached.value == 5 * 4 * 6
